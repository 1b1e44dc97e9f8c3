// export_host.cpp -- lm_export_frames' host-side code driven without a GPU (tests/test_export_cpu.py; g++, plain and under ASan / UBSan):
// the rule's shared functions (csrc/lm_draw.h: exactly what k_export runs), the descriptor and primitive checks (csrc/lm_export_check.cpp)
// and the tile planner (lmh::plan_export, csrc/lm_host.cpp).  It computes and dumps; the pytest compares with tests/export_reference.py and
// with the numbers written out in include/linemod_hip.h.
//   pins                               ring / segment pixel counts, the NV12 triples of white and red, blend values, all 2^24 blends
//   cover W H in out                   in: "kind x0 y0 x1 y1 t" per line -> out: W * H coverage bytes per line
//   products in out                    in: "x0 y0 x1 y1 t x y" per line -> out: "s L2 cross 4cross^2 t^2L2 covered" per line (segment)
//   plan W H frames max in out         in: `frames` lines "flip sx sy", then "kind frame x0 y0 x1 y1 t" per line -> out: the plan
//   yuv in out                         in: "row a b c" per line -> out: "luma(a, b, c) chroma_u(a, b, c) chroma_v(a, b, c)"
//   refuse in out                      in: one check per line (see below) -> out: the refusal, or "OK ..."
// Prints "OK <lines answered>".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "lm_draw.h"
#include "lm_export_check.h"
#include "lm_host.h"

static lmw::Rec rec_of(int kind, int x0, int y0, int x1, int y1, int t) { return lmw::make_rec(kind, x0, y0, x1, y1, t, 0xFF0000FFu); }

static int count(const lmw::Rec& r, int w, int h) {
    int n = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) n += lmw::covered(r, x, y) ? 1 : 0;
    return n;
}

static int pins() {
    for (int r = 0; r <= 5; ++r) std::printf("ring %d %d\n", r, count(rec_of(lmw::RING, 16, 16, r, 0, 1), 32, 32));
    for (int t = 1; t <= 2; ++t) std::printf("segment %d %d\n", t, count(rec_of(lmw::SEGMENT, 2, 2, 10, 5, t), 32, 32));
    for (int t = 1; t <= 3; ++t) std::printf("zero %d %d\n", t, count(rec_of(lmw::SEGMENT, 7, 9, 7, 9, t), 32, 32));
    for (int row = 0; row < 4; ++row) {
        const lmw::FwdCoef c = lmw::fwd_coef(row);
        std::printf("white %d %d %d %d\n", row, lmw::luma(255, 255, 255, c), lmw::chroma_u(1020, 1020, 1020, c), lmw::chroma_v(1020, 1020, 1020, c));
        std::printf("red %d %d %d %d\n", row, lmw::luma(255, 0, 0, c), lmw::chroma_u(1020, 0, 0, c), lmw::chroma_v(1020, 0, 0, c));
    }
    const unsigned as[6] = {0, 1, 127, 128, 254, 255}, cs[4] = {0, 1, 200, 255}, ps[4] = {0, 37, 254, 255};
    for (unsigned a : as)
        for (unsigned c : cs)
            for (unsigned p : ps) std::printf("blend %u %u %u %u\n", a, c, p, lmw::blend(c, p, a));
    // round-to-nearest of (c (255 - a) + p a) / 255 over all 2^24 triples (no tie exists: 255 is odd)
    long long bad = 0;
    for (unsigned a = 0; a < 256; ++a)
        for (unsigned c = 0; c < 256; ++c)
            for (unsigned p = 0; p < 256; ++p) bad += lmw::blend(c, p, a) != (2 * (c * (255 - a) + p * a) + 255) / 510;
    std::printf("blendall %lld\n", bad);
    // the packed pixel form
    std::printf("pixel %u\n", lmw::blend_pixel(0x00102030u, 0x80FF8000u));
    std::printf("OK 1\n");
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "pins") return pins();
    if (mode == "cover" && argc == 6) {
        const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
        std::ifstream in(argv[4]);
        std::ofstream out(argv[5], std::ios::binary);
        int n = 0, kind, x0, y0, x1, y1, t;
        std::vector<char> m((size_t)w * h);
        while (in >> kind >> x0 >> y0 >> x1 >> y1 >> t) {
            const lmw::Rec r = rec_of(kind, x0, y0, x1, y1, t);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) m[(size_t)y * w + x] = lmw::covered(r, x, y) ? 1 : 0;
            out.write(m.data(), (std::streamsize)m.size());
            ++n;
        }
        std::printf("OK %d\n", n);
        return 0;
    }
    if (mode == "products" && argc == 4) {
        std::ifstream in(argv[2]);
        std::ofstream out(argv[3]);
        int n = 0, x0, y0, x1, y1, t, x, y;
        while (in >> x0 >> y0 >> x1 >> y1 >> t >> x >> y) {
            const lmw::Rec r = rec_of(lmw::SEGMENT, x0, y0, x1, y1, t);
            const int wx = x - r.x0, wy = y - r.y0, s = wx * r.a + wy * r.b;
            const long long cross = (long long)(wx * r.b - wy * r.a);
            out << s << " " << r.c << " " << cross << " " << 4 * cross * cross << " " << r.k64 << " " << (lmw::segment_covered(r, x, y) ? 1 : 0) << "\n";
            ++n;
        }
        std::printf("OK %d\n", n);
        return 0;
    }
    if (mode == "plan" && argc == 8) {
        const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), frames = std::atoi(argv[4]);
        const size_t max_entries = (size_t)std::atoll(argv[5]);
        std::ifstream in(argv[6]);
        std::ofstream out(argv[7]);
        std::vector<lmh::ExportUndo> undo((size_t)frames);
        for (auto& o : undo) in >> o.flip_x >> o.shift_x >> o.shift_y;
        std::vector<lm_draw_prim> prims;
        lm_draw_prim p = {};
        while (in >> p.kind >> p.frame >> p.x0 >> p.y0 >> p.x1 >> p.y1 >> p.thickness) { p.b = 1; p.g = 2; p.r = 3; p.a = 255; prims.push_back(p); }
        lmh::ExportPlan plan;
        const bool ok = lmh::plan_export(w, h, frames, undo.data(), prims.data(), prims.size(), max_entries, plan);
        out << (ok ? "ok" : "overflow") << " " << plan.tiles_x << " " << plan.tiles_y << " " << plan.entries << " " << lmh::EXPORT_TILE_W << " "
            << lmh::EXPORT_TILE_H << " " << plan.recs.size() << "\n";
        for (unsigned v : plan.tile_off) out << v << " ";
        out << "\n";
        for (unsigned v : plan.idx) out << v << " ";
        out << "\n";
        // the records' boxes, as the kernel's per-lane rejection reads them
        for (const lmw::Rec& r : plan.recs) out << r.bx0 << " " << r.by0 << " " << r.bx1 << " " << r.by1 << " ";
        out << "\n";
        std::printf("OK %zu\n", prims.size());
        return 0;
    }
    if (mode == "yuv" && argc == 4) {
        std::ifstream in(argv[2]);
        std::ofstream out(argv[3]);
        int n = 0, row, a, b, c;
        while (in >> row >> a >> b >> c) {
            const lmw::FwdCoef k = lmw::fwd_coef(row);
            out << lmw::luma(a, b, c, k) << " " << lmw::chroma_u(a, b, c, k) << " " << lmw::chroma_v(a, b, c, k) << "\n";
            ++n;
        }
        std::printf("OK %d\n", n);
        return 0;
    }
    if (mode == "refuse" && argc == 4) {
        // counts  dst_null n_slots prims_null n_prims
        // frame   W H
        // image   W H frame data row_stride plane_stride width height format crop_x crop_y
        // prim    n_frames k kind frame x0 y0 x1 y1 t
        // overlap W H n, then per image: data row_stride plane_stride width height format crop_x crop_y
        std::ifstream in(argv[2]);
        std::ofstream out(argv[3]);
        std::string line;
        int n = 0;
        const auto read_image = [](std::istream& s, lm_image_desc* im) {
            unsigned long long data;
            long long rs, ps;
            s >> data >> rs >> ps >> im->width >> im->height >> im->format >> im->crop_x >> im->crop_y;
            im->data = reinterpret_cast<const void*>((uintptr_t)data); im->row_stride = rs; im->plane_stride = ps; im->scale = 0.0f;
        };
        while (std::getline(in, line)) {
            std::istringstream s(line);
            std::string what;
            s >> what;
            std::string r = "?";
            if (what == "counts") {
                int dn, ns, pn; unsigned long long np;
                s >> dn >> ns >> pn >> np;
                r = lmc::check_export_counts(dn != 0, ns, pn != 0, (size_t)np);
            } else if (what == "frame") {
                int w, h;
                s >> w >> h;
                r = lmc::check_export_frame(w, h);
            } else if (what == "image") {
                int w, h, frame;
                s >> w >> h >> frame;
                lm_image_desc im = {};
                read_image(s, &im);
                LmExportImage e = {};
                r = lmc::check_export_image(w, h, im, frame, &e);
                if (r.empty()) r = "OK " + std::to_string(e.kind) + " " + std::to_string(e.swap_rb) + " " + std::to_string(e.matrix) + " " +
                                   std::to_string(e.row_stride) + " " + std::to_string(e.plane_stride) + " " + std::to_string(e.crop_x) + " " + std::to_string(e.crop_y);
            } else if (what == "prim") {
                int nf; unsigned long long k;
                lm_draw_prim p = {};
                s >> nf >> k >> p.kind >> p.frame >> p.x0 >> p.y0 >> p.x1 >> p.y1 >> p.thickness;
                r = lmc::check_export_prim(p, (size_t)k, nf);
            } else if (what == "overlap") {
                int w, h, ni;
                s >> w >> h >> ni;
                std::vector<LmExportImage> es((size_t)ni);
                r.clear();
                for (int i = 0; i < ni && r.empty(); ++i) {
                    lm_image_desc im = {};
                    read_image(s, &im);
                    r = lmc::check_export_image(w, h, im, i, &es[(size_t)i]);
                }
                if (r.empty()) r = lmc::check_export_overlap(w, h, es.data(), ni);
            }
            out << (r.empty() ? std::string("OK") : r) << "\n";
            ++n;
        }
        std::printf("OK %d\n", n);
        return 0;
    }
    std::fprintf(stderr, "usage: export_host pins | cover | products | plan | yuv | refuse ...\n");
    return 2;
}
