// ingest_check_host.cpp -- csrc/lm_ingest_check.cpp on the host: the descriptor check of the ingest family, with no detector and no GPU.  Built
// by tests/test_ingest_check_cpu.py with g++, plain and under ASan / UBSan, and compared there with tables written out in the test.
//   ingest_check_host cases IN OUT     IN: one case per line,
//           GEOM ROLE WHOLE  CW CH  AW AH BW BH  FLIP SHIFT_X  FRAME  DATA ROW_STRIDE PLANE_STRIDE WIDTH HEIGHT FORMAT CROP_X CROP_Y SCALE
//       GEOM plain | rect | raw; ROLE c | d (raw: ignored); CW x CH the detector's frame; A the source camera (rect) or the registration's depth
//       camera (raw), B the ideal camera (rect) or the colour camera (raw); DATA an address that is never read.
//       OUT: per case "1|<refusal>" or "0|kind swap_rb aligned row_stride plane_stride crop_x crop_y scale_bits matrix data" (matrix: -1
//       where the caller passes no matrix, as for a depth image)
//   ingest_check_host sweep GEOM FORMAT NPLANE NCROP SHIFT OUT     window 32 x 16 in a 64 x 32 source (= camera A; B is 96 x 48): one byte per
//       (data % 16, row_stride % 16, plane_stride % 16 < NPLANE, crop_x < NCROP, shift_x in -SHIFT .. SHIFT, flip_x), in that nesting
//       order: the `aligned` flag, or 2 where the image is refused
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "lm_ingest_check.h"

static lmc::Geometry geometry(const std::string& geom, bool depth, bool whole, int cw, int ch, int aw, int ah, int bw, int bh) {
    lm_config c = lm_config();
    c.width = cw; c.height = ch;
    if (geom == "rect") {
        lm_rectification_desc r = lm_rectification_desc();
        r.source.width = aw; r.source.height = ah; r.ideal.width = bw; r.ideal.height = bh;
        return lmc::rectified(c, r, depth ? lmc::DEPTH : lmc::COLOUR, whole);
    }
    if (geom == "raw") {
        lm_registration_desc r = lm_registration_desc();
        r.depth.width = aw; r.depth.height = ah; r.colour.width = bw; r.colour.height = bh;
        return lmc::raw_depth(c, r, whole);
    }
    return lmc::plain(c, depth ? lmc::DEPTH : lmc::COLOUR);
}

static int cases(const char* in_path, const char* out_path) {
    std::ifstream in(in_path);
    std::ofstream out(out_path);
    if (!in || !out) return 2;
    std::string line;
    size_t n = 0;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string geom, role, scale;
        int whole, cw, ch, aw, ah, bw, bh, frame;
        unsigned long long data;
        lm_ingest_opts o = lm_ingest_opts();
        lm_image_desc im = lm_image_desc();
        if (!(s >> geom >> role >> whole >> cw >> ch >> aw >> ah >> bw >> bh >> o.flip_x >> o.shift_x >> frame >> data >> im.row_stride >> im.plane_stride >>
              im.width >> im.height >> im.format >> im.crop_x >> im.crop_y >> scale)) return 3;
        im.data = reinterpret_cast<const void*>(static_cast<uintptr_t>(data));
        im.scale = std::strtof(scale.c_str(), nullptr);
        const bool depth = role == "d";
        LmIngestImage img;
        std::memset(&img, 0xAB, sizeof(img));       // (the check fills every field)
        int matrix = -1;
        const std::string refusal = lmc::check_image(geometry(geom, depth, whole != 0, cw, ch, aw, ah, bw, bh), im, frame, o, &img, depth || geom == "raw" ? nullptr : &matrix);
        if (!refusal.empty()) out << "1|" << refusal << "\n";
        else {
            uint32_t bits;
            std::memcpy(&bits, &img.scale, 4);
            out << "0|" << img.kind << " " << img.swap_rb << " " << img.aligned << " " << img.row_stride << " " << img.plane_stride << " " << img.crop_x << " "
                << img.crop_y << " " << bits << " " << matrix << " " << static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(img.data)) << "\n";
        }
        ++n;
    }
    std::printf("OK %zu\n", n);
    return 0;
}

static int sweep(const std::string& geom, int format, int nplane, int ncrop, int shift, const char* out_path) {
    const bool depth = format == LM_PIX_DEPTH_U16 || format == LM_PIX_DEPTH_F32;
    const lmc::Geometry g = geometry(geom, depth, false, 32, 16, 64, 32, 96, 48);
    std::vector<unsigned char> flags;
    for (int a = 0; a < 16; ++a)
        for (int r = 0; r < 16; ++r)
            for (int p = 0; p < nplane; ++p)
                for (int cx = 0; cx < ncrop; ++cx)
                    for (int sx = -shift; sx <= shift; ++sx)
                        for (int flip = 0; flip < 2; ++flip) {
                            lm_image_desc im = lm_image_desc();
                            im.data = reinterpret_cast<const void*>(static_cast<uintptr_t>(0x10000 + a));
                            im.row_stride = 256 + r; im.plane_stride = 8192 + p;
                            im.width = 64; im.height = 32; im.format = format; im.crop_x = cx; im.crop_y = 3; im.scale = 1.0f;
                            const lm_ingest_opts o = {flip, sx, 0};
                            LmIngestImage img;
                            std::memset(&img, 0xAB, sizeof(img));
                            const std::string refusal = lmc::check_image(g, im, 0, o, &img, nullptr);
                            flags.push_back(refusal.empty() ? (unsigned char)img.aligned : 2);
                        }
    FILE* f = std::fopen(out_path, "wb");
    if (!f) return 2;
    std::fwrite(flags.data(), 1, flags.size(), f);
    std::fclose(f);
    std::printf("OK %zu\n", flags.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "cases")) return cases(argv[2], argv[3]);
    if (argc == 8 && !std::strcmp(argv[1], "sweep")) return sweep(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]), argv[7]);
    std::fprintf(stderr, "usage: ingest_check_host cases IN OUT | sweep GEOM FORMAT NPLANE NCROP SHIFT OUT\n");
    return 2;
}
