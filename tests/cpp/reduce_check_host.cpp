// reduce_check_host.cpp -- the host-only checks of the reduced route (csrc/lm_ingest_check.cpp: lmc::check_reduction, and lmc::check_image
// against lmc::reduced), with no detector and no GPU.  Built by tests/test_reduce_cpu.py with g++ under ASan / UBSan.
//   reduce_check_host desc NUM_X DEN_X NUM_Y DEN_Y APPLY RULE          "1|<refusal>" or "0|num_x den_x num_y den_y apply rule" (lowest terms)
//   reduce_check_host image ROLE WHOLE CW CH NUM_X DEN_X NUM_Y DEN_Y APPLY  DATA ROW_STRIDE PLANE_STRIDE WIDTH HEIGHT FORMAT CROP_X CROP_Y
//       ROLE c | d; CW x CH the detector's frame; DATA an address that is never read.
//       "1|<refusal>" or "0|kind aligned crop_x crop_y src_w src_h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "lm_ingest_check.h"

int main(int argc, char** argv) {
    if (argc == 8 && !std::strcmp(argv[1], "desc")) {
        const lm_reduction_desc in = {std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7])};
        lm_reduction_desc out = {-1, -1, -1, -1, -1, -1};
        const std::string refusal = lmc::check_reduction(in, &out);
        if (!refusal.empty()) std::printf("1|%s\n", refusal.c_str());
        else std::printf("0|%d %d %d %d %d %d\n", out.num_x, out.den_x, out.num_y, out.den_y, out.apply, out.depth_rule);
        return 0;
    }
    if (argc == 19 && !std::strcmp(argv[1], "image")) {
        lm_config c = lm_config();
        c.width = std::atoi(argv[4]); c.height = std::atoi(argv[5]);
        const lm_reduction_desc red = {std::atoi(argv[6]), std::atoi(argv[7]), std::atoi(argv[8]), std::atoi(argv[9]), std::atoi(argv[10]), 0};
        lm_image_desc im = lm_image_desc();
        im.data = reinterpret_cast<const void*>(static_cast<uintptr_t>(std::strtoull(argv[11], nullptr, 0)));
        im.row_stride = std::atoll(argv[12]); im.plane_stride = std::atoll(argv[13]);
        im.width = std::atoi(argv[14]); im.height = std::atoi(argv[15]); im.format = std::atoi(argv[16]); im.crop_x = std::atoi(argv[17]); im.crop_y = std::atoi(argv[18]);
        im.scale = 1.0f;
        const bool depth = argv[2][0] == 'd';
        LmIngestImage img;
        std::memset(&img, 0xAB, sizeof(img));
        int matrix = -1;
        const std::string refusal = lmc::check_image(lmc::reduced(c, red, depth ? lmc::DEPTH : lmc::COLOUR, std::atoi(argv[3]) != 0), im, 0, lm_ingest_opts{0, 0, 0}, &img,
                                                     depth ? nullptr : &matrix);
        if (!refusal.empty()) std::printf("1|%s\n", refusal.c_str());
        else std::printf("0|%d %d %d %d %d %d\n", img.kind, img.aligned, img.crop_x, img.crop_y, img.src_w, img.src_h);
        return 0;
    }
    std::fprintf(stderr, "usage: reduce_check_host desc ... | image ...\n");
    return 2;
}
