// ingest_float_host.cpp -- csrc/lm_ingest_float.h on the host: the code k_ingest_float runs per lane (lane_window, load_span, the element
// unpacking, to_u8) and the two conversions of lm_export_frames' float destinations, with the memory read replaced by a loader that CHECKS
// every 16-byte load.  Built by tests/test_ingest_float_cpu.py with g++ -ffp-contract=off, plain and under ASan / UBSan; its answers are
// compared there, byte for byte, with tests/ingest_float_reference.py (numpy).  Never loaded into Python.
//   ingest_float_host h8 SCALE_BITS OUT          to_u8 of all 65536 binary16 bit patterns: 65536 bytes
//   ingest_float_host u8 SCALE_BITS IN OUT       IN: binary32 bit patterns (u32); OUT: one byte each
//   ingest_float_host export SCALE_BITS OUT      the 256 bytes as binary32 bits (256 u32), then as binary16 bits (256 u16)
//   ingest_float_host frames IN OUT              IN: cases, each 14 int32 (format, w, h, src_w, src_h, crop_x, crop_y, flip_x, shift_x, shift_y,
//       offset, row_stride, plane_stride, nbytes), the scale (float) and nbytes bytes: a heap block that ENDS where the source ends (ASan
//       guards the byte behind), the source's pixel (0, 0) `offset` bytes into it (malloc's blocks are 16-byte aligned: offset % 16 is the
//       misalignment class of `data`).  The descriptor goes through lmc::check_image (lm_ingest_check.cpp), every lane of the w x h frame
//       through lmf::float_lane_pixels and k_ingest's arrange.  Checked per lane: every load is 16-byte aligned, and is the `safe` block or
//       holds at least one byte of an element a kept pixel needs (computed here from the layout's definition); the bytes a load holds
//       outside the heap block and the safe block's content are poison.  OUT: w * h * 3 bytes per case, B G R.
//   ingest_float_host export_check IN OUT        csrc/lm_export_check.cpp.  IN, per line: "image W H FRAME DATA ROW_STRIDE PLANE_STRIDE WIDTH
//       HEIGHT FORMAT CROP_X CROP_Y SCALE_BITS", or "overlap W H" followed by two such image tails (DATA ..).  OUT, per line: the refusal,
//       or "OK kind swap_rb es scale_bits plane_stride" / "OK"
// Prints "OK <count>"; any failure prints the case and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <vector>

#include "lm_export_check.h"
#include "lm_ingest_check.h"

using lmi::addr_t;
using lmi::u32;

static float float_of(const char* bits) {
    const u32 b = (u32)strtoul(bits, nullptr, 0);
    float f;
    memcpy(&f, &b, 4);
    return f;
}

static bool write_all(const char* path, const void* p, size_t n) {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

static bool g_failed = false;
static char g_case[256];
static unsigned long long g_loads = 0, g_safe_loads = 0;
static void fail(const char* what) {
    if (!g_failed) printf("FAILED %s: %s\n", g_case, what);
    g_failed = true;
}

struct Range { addr_t lo, hi; };
struct CheckedLoad {
    addr_t alloc_lo, alloc_hi, safe;
    const std::vector<Range>* need;
    lmi::Vec16 operator()(addr_t p) const {
        ++g_loads;
        if (p % 16) fail("a load that is not 16-byte aligned");
        if (p == safe) { ++g_safe_loads; return lmi::Vec16{0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu}; }
        bool needed = false;
        for (const Range& r : *need) needed = needed || (r.lo < p + 16 && r.hi > p);
        if (!needed) fail("a load outside `safe` that holds no byte a kept pixel needs");
        uint8_t b[16];
        for (int i = 0; i < 16; ++i) b[i] = (p + i >= alloc_lo && p + i < alloc_hi) ? *reinterpret_cast<const uint8_t*>((uintptr_t)(p + i)) : 0xA5;
        lmi::Vec16 v;
        memcpy(&v, b, 16);
        return v;
    }
};

static int frames(const char* in_path, const char* out_path) {
    FILE* in = fopen(in_path, "rb");
    FILE* out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    alignas(16) static uint8_t safe_block[16];
    const addr_t safe = (addr_t)(uintptr_t)safe_block;
    unsigned long long n_cases = 0;
    int32_t hd[14];
    while (fread(hd, 4, 14, in) == 14) {
        float scale;
        if (fread(&scale, 4, 1, in) != 1) return 3;
        const int format = hd[0], w = hd[1], h = hd[2], flip = hd[7], offset = hd[10];
        const size_t nbytes = (size_t)hd[13];
        uint8_t* block = static_cast<uint8_t*>(malloc(nbytes));
        if (!block || fread(block, 1, nbytes, in) != nbytes) return 3;
        lm_config cfg = lm_config();
        cfg.width = w; cfg.height = h;
        lm_image_desc im = lm_image_desc();
        im.data = block + offset; im.row_stride = hd[11]; im.plane_stride = hd[12]; im.width = hd[3]; im.height = hd[4];
        im.format = format; im.crop_x = hd[5]; im.crop_y = hd[6]; im.scale = scale;
        lm_ingest_opts o = {flip, hd[8], hd[9]};
        LmIngestImage img;
        int matrix = -1;
        snprintf(g_case, sizeof g_case, "format 0x%x offset %d stride %d crop (%d, %d) flip %d shift (%d, %d)", format, offset, hd[11], hd[5], hd[6], flip, hd[8], hd[9]);
        const std::string refusal = lmc::check_image(lmc::plain(cfg, lmc::COLOUR), im, 0, o, &img, &matrix);
        if (!refusal.empty()) { fail(refusal.c_str()); return 1; }
        if (lm_ingest_family(img.kind) != LM_INGEST_FAMILY_FLOAT) { fail("not the float family's kind"); return 1; }
        lmf::Src src;
        src.data = (addr_t)(uintptr_t)img.data; src.row_stride = img.row_stride; src.plane_stride = img.plane_stride;
        src.crop_x = img.crop_x; src.crop_y = img.crop_y; src.kind = img.kind; src.swap_rb = img.swap_rb; src.aligned = img.aligned != 0; src.scale = img.scale;
        // the layout's definition, for the bytes a kept pixel needs
        const int es = (format & 0x10) ? 2 : 4, lay = format & 15, nch = lay <= 1 ? 3 : lay <= 3 ? 4 : 1;
        std::vector<uint8_t> frame((size_t)w * h * 3);
        for (int y = 0; y < h; ++y)
            for (int x0 = 0; x0 < w; x0 += 16) {
                std::vector<Range> need;
                for (int j = 0; j < 16; ++j) {
                    const int xs = x0 + j - o.shift_x, ys = y - o.shift_y;
                    if (xs < 0 || xs >= w || ys < 0 || ys >= h) continue;
                    const long long c = im.crop_x + (flip ? w - 1 - xs : xs), r = im.crop_y + ys;
                    const addr_t px = (addr_t)(uintptr_t)im.data + (addr_t)(r * im.row_stride + c * es * nch);
                    if (lay == 4 || lay == 5) for (int p = 0; p < 3; ++p) need.push_back({px + (addr_t)(p * im.plane_stride), px + (addr_t)(p * im.plane_stride) + es});
                    else need.push_back({px, px + (addr_t)(es * nch)});          // (the ignored alpha is a byte of the kept pixel too: inside the source)
                }
                const lmi::Lane L = lmi::lane_window(w, h, x0, y, flip != 0, o.shift_x, o.shift_y);
                u32 P[16];
                lmf::float_lane_pixels(src, L, safe, CheckedLoad{(addr_t)(uintptr_t)block, (addr_t)(uintptr_t)block + nbytes, safe, &need}, P);
                for (int j = 0; j < 16; ++j) {          // k_ingest's arrange
                    const int k = flip ? 15 - j : j;
                    const u32 px = (k >= L.klo && k < L.khi) ? P[k] : 0u;
                    uint8_t* q = &frame[((size_t)y * w + x0 + j) * 3];
                    q[0] = (uint8_t)px; q[1] = (uint8_t)(px >> 8); q[2] = (uint8_t)(px >> 16);
                }
                if (g_failed) return 1;
            }
        if (fwrite(frame.data(), 1, frame.size(), out) != frame.size()) return 2;
        free(block);
        ++n_cases;
    }
    fclose(in);
    if (fclose(out)) return 2;
    if (g_safe_loads == 0 || g_safe_loads == g_loads) { printf("FAILED: %llu of %llu loads went to the safe block\n", g_safe_loads, g_loads); return 1; }
    printf("OK %llu cases, %llu loads, %llu of them to the safe block\n", n_cases, g_loads, g_safe_loads);
    return 0;
}

static bool read_image(std::istream& s, lm_image_desc* im) {
    unsigned long long data;
    long long rs, ps;
    std::string scale;
    if (!(s >> data >> rs >> ps >> im->width >> im->height >> im->format >> im->crop_x >> im->crop_y >> scale)) return false;
    im->data = reinterpret_cast<const void*>((uintptr_t)data); im->row_stride = rs; im->plane_stride = ps; im->scale = float_of(scale.c_str());
    return true;
}

static int export_check(const char* in_path, const char* out_path) {
    std::ifstream in(in_path);
    std::ofstream out(out_path);
    if (!in || !out) return 2;
    std::string line;
    int n = 0;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string what;
        int w, h;
        s >> what >> w >> h;
        if (what == "image") {
            int frame;
            lm_image_desc im = lm_image_desc();
            s >> frame;
            if (!read_image(s, &im)) return 3;
            LmExportImage e;
            const std::string r = lmc::check_export_image(w, h, im, frame, &e);
            if (!r.empty()) out << r << "\n";
            else out << "OK " << e.kind << " " << e.swap_rb << " " << e.es << " " << lmf::as_bits(e.scale) << " " << e.plane_stride << "\n";
        } else if (what == "overlap") {
            lm_image_desc im[2] = {lm_image_desc(), lm_image_desc()};
            LmExportImage e[2];
            for (int k = 0; k < 2; ++k)
                if (!read_image(s, &im[k]) || !lmc::check_export_image(w, h, im[k], k, &e[k]).empty()) return 3;
            const std::string r = lmc::check_export_overlap(w, h, e, 2);
            out << (r.empty() ? "OK" : r) << "\n";
        } else return 3;
        ++n;
    }
    printf("OK %d\n", n);
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "h8" && argc == 4) {
        const float scale = float_of(argv[2]);
        std::vector<uint8_t> out(65536);
        for (u32 b = 0; b < 65536u; ++b) out[b] = (uint8_t)lmf::to_u8(lmf::half_to_float(b), scale);
        if (!write_all(argv[3], out.data(), out.size())) return 2;
        printf("OK 65536\n");
        return 0;
    }
    if (mode == "u8" && argc == 5) {
        const float scale = float_of(argv[2]);
        FILE* in = fopen(argv[3], "rb");
        if (!in) return 2;
        std::vector<uint8_t> out;
        u32 b;
        while (fread(&b, 4, 1, in) == 1) out.push_back((uint8_t)lmf::to_u8(lmf::as_float(b), scale));
        fclose(in);
        if (!write_all(argv[4], out.data(), out.size())) return 2;
        printf("OK %zu\n", out.size());
        return 0;
    }
    if (mode == "export" && argc == 4) {
        const float scale = float_of(argv[2]);
        uint8_t out[256 * 6];
        for (u32 c = 0; c < 256u; ++c) {
            const u32 f = lmf::from_u8_f32(c, scale);
            const uint16_t hf = (uint16_t)lmf::from_u8_f16(c, scale);
            memcpy(out + 4 * c, &f, 4);
            memcpy(out + 1024 + 2 * c, &hf, 2);
        }
        if (!write_all(argv[3], out, sizeof out)) return 2;
        printf("OK 256\n");
        return 0;
    }
    if (mode == "frames" && argc == 4) return frames(argv[2], argv[3]);
    if (mode == "export_check" && argc == 4) return export_check(argv[2], argv[3]);
    printf("usage: ingest_float_host h8 | u8 | export | frames | export_check ...\n");
    return 2;
}
