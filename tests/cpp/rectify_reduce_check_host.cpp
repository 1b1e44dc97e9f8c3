// rectify_reduce_check_host.cpp -- the host-only descriptor check of the rectified and reduced route (csrc/lm_ingest_check.cpp:
// lmc::check_image against lmc::rectified_reduced), with no detector and no GPU.  Built by tests/test_rectify_reduce_cpu.py with g++ under
// ASan / UBSan.
//   rectify_reduce_check_host image ROLE WHOLE CW CH  SW SH IW IH  NUM_X DEN_X NUM_Y DEN_Y APPLY  DATA ROW_STRIDE PLANE_STRIDE WIDTH HEIGHT FORMAT CROP_X CROP_Y
//       ROLE c | d; CW x CH the detector's frame; SW x SH the source camera, IW x IH the ideal camera; the ratio in lowest terms; DATA an
//       address that is never read.
//       "1|<refusal>" or "0|kind aligned crop_x crop_y src_w src_h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "lm_ingest_check.h"

int main(int argc, char** argv) {
    if (argc == 23 && !std::strcmp(argv[1], "image")) {
        lm_config c = lm_config();
        c.width = std::atoi(argv[4]); c.height = std::atoi(argv[5]);
        lm_rectification_desc rect = lm_rectification_desc();
        rect.source.width = std::atoi(argv[6]); rect.source.height = std::atoi(argv[7]);
        rect.ideal.width = std::atoi(argv[8]); rect.ideal.height = std::atoi(argv[9]);
        const lm_reduction_desc red = {std::atoi(argv[10]), std::atoi(argv[11]), std::atoi(argv[12]), std::atoi(argv[13]), std::atoi(argv[14]), 0};
        lm_image_desc im = lm_image_desc();
        im.data = reinterpret_cast<const void*>(static_cast<uintptr_t>(std::strtoull(argv[15], nullptr, 0)));
        im.row_stride = std::atoll(argv[16]); im.plane_stride = std::atoll(argv[17]);
        im.width = std::atoi(argv[18]); im.height = std::atoi(argv[19]); im.format = std::atoi(argv[20]); im.crop_x = std::atoi(argv[21]); im.crop_y = std::atoi(argv[22]);
        im.scale = 1.0f;
        const bool depth = argv[2][0] == 'd';
        LmIngestImage img;
        std::memset(&img, 0xAB, sizeof(img));
        int matrix = -1;
        const std::string refusal = lmc::check_image(lmc::rectified_reduced(c, rect, red, depth ? lmc::DEPTH : lmc::COLOUR, std::atoi(argv[3]) != 0), im, 0,
                                                     lm_ingest_opts{0, 0, 0}, &img, depth ? nullptr : &matrix);
        if (!refusal.empty()) std::printf("1|%s\n", refusal.c_str());
        else std::printf("0|%d %d %d %d %d %d\n", img.kind, img.aligned, img.crop_x, img.crop_y, img.src_w, img.src_h);
        return 0;
    }
    std::fprintf(stderr, "usage: rectify_reduce_check_host image ...\n");
    return 2;
}
