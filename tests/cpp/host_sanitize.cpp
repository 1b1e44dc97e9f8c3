// Sanitizer driver for the host-only parts of liblinemod_hip.so (csrc/lm_yaml.cpp, lm_host.cpp, lm_extract.cpp): built by
// tests/test_sanitize.py with g++ -fsanitize=address,undefined (CPU build only; GPU ASan is not available on the pool).
// lm_load_yaml / lm_load_bank parse files this library did not write (HighLevelLinemod.cpp:292-303 reads whatever
// linemod_templates.yml.gz is lying around), so valid files are mutated -- truncated, bytes flipped, spans deleted or
// duplicated, numbers replaced by absurd ones -- and every mutant goes through the parser, the template loader, the
// device-bank builder and the hull table.  A mutant may be rejected (false + message) or accepted; it must never crash,
// read out of bounds, overflow, or hang.
// usage: host_sanitize <opencv_style_templates.yml> <iterations> <seed> <scratch dir>
#include <cstdint>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../line-mod-pipeline_amd/csrc/lm_extract.h"
#include "../../line-mod-pipeline_amd/csrc/lm_host.h"
#include "../../line-mod-pipeline_amd/csrc/lm_yaml.h"

static lm_config make_cfg(int M) {
    lm_config c;
    std::memset(&c, 0, sizeof(c));
    c.width = 640; c.height = 480; c.num_modalities = M; c.pyramid_levels = 2;
    c.T[0] = M == 2 ? 5 : 2; c.T[1] = 8;
    c.weak_threshold = 10.f; c.num_features = 63; c.strong_threshold = 55.f;
    c.distance_threshold = 2000; c.difference_threshold = 50; c.depth_num_features = 63; c.extract_threshold = 2;
    c.shard_rank = 0; c.shard_size = 1;
    return c;
}

static void make_geom(const lm_config& c, LmLevelGeom* geom) {   // as lm_create does
    int w = c.width, h = c.height;
    for (int l = 0; l < c.pyramid_levels; ++l) {
        if (l > 0) { w /= 2; h /= 2; }
        LmLevelGeom& g = geom[l];
        std::memset(&g, 0, sizeof(g));
        g.w = w; g.h = h; g.T = c.T[l]; g.W = w / g.T; g.H = h / g.T; g.wh = (u32)g.W * (u32)g.H;
        g.spread_only = l + 1 < c.pyramid_levels; g.nibble = g.spread_only ? 0 : 1;
        const size_t pad = ((size_t)g.wh + 16 * (size_t)g.W + 2 * LM_SCAN_CHUNK + 64 + 255) / 256 * 256;
        const size_t ori = ((((size_t)g.T * g.T * g.wh) >> g.nibble) + 255) / 256 * 256 + pad;
        const size_t plane = g.nibble ? (((size_t)g.T * g.T * g.wh + 7) / 8 + ((size_t)g.wh + 64 * 128) / 8 + 64 + 255) / 256 * 256 : 0;   // r05: the miss planes
        g.ori_stride = (u32)ori; g.plane_ori = (u32)plane; g.mod_stride = (u32)(g.spread_only ? ori : 8 * ori + 8 * plane);
        g.zero_off = (u32)((size_t)c.num_modalities * g.mod_stride); g.arena_bytes = g.zero_off + (u32)pad;
    }
}

static void digest(const lmh::Bank& bank, const lm_config& cfg) {
    LmLevelGeom geom[LM_MAX_LEVELS];
    make_geom(cfg, geom);
    lmh::DeviceBankHost hb;
    std::string err;
    // every order of the scan lists (LM_TUNE_SCAN_LIST_ORDER): each must be a permutation of the ascending lists, list by list
    std::vector<u32> base;
    size_t fpad = 0;
    for (int order = 0; order <= 3; ++order) {
        if (!lmh::build_device_bank(bank, cfg, geom, hb, order, err)) return;
        if (order == 0) { base = hb.scan_off; fpad = (size_t)hb.fpad; continue; }
        if (hb.scan_off.size() != base.size() || fpad == 0) { std::printf("scan list order %d changes the list sizes\n", order); std::abort(); }
        for (size_t at = 0; at + fpad <= base.size(); at += fpad) {
            std::vector<u32> a(base.begin() + (ptrdiff_t)at, base.begin() + (ptrdiff_t)(at + fpad)), b(hb.scan_off.begin() + (ptrdiff_t)at, hb.scan_off.begin() + (ptrdiff_t)(at + fpad));
            std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end());
            if (a != b) { std::printf("scan list order %d is not a permutation of the ascending list at %zu\n", order, at); std::abort(); }
        }
    }
    // r05, the bit-plane scan's lists (order 3 is in hb): per template the in-bounds features of all modalities once, every bit offset inside a
    // miss plane of the right modality and orientation and at the same position as its nibble offset; padding = the zero block; work items for L
    // lanes per frame cover every template's positions exactly once
    {
        const LmLevelGeom& g = geom[cfg.pyramid_levels - 1];
        const int M = cfg.num_modalities;
        const size_t nt = hb.scan_P.size();
        if (hb.fpad1 <= 0 || hb.fpad1 % 8 || hb.off1.size() != nt * (size_t)hb.fpad1 || hb.offn.size() != hb.off1.size() || hb.offs3.size() != hb.off1.size()) { std::printf("bit-plane lists have the wrong shape\n"); std::abort(); }
        for (size_t t = 0; t < nt; ++t) {
            const int cnt = hb.scan_n[t];
            int F = 0;
            std::vector<u32> want;
            for (int m = 0; m < M; ++m) {
                const int k = (cnt >> (8 + 8 * m)) & 0xFF;
                for (int q = 0; q < k; ++q) want.push_back(hb.scan_off[(t * M + m) * (size_t)hb.fpad + q]);
                F += k;
            }
            for (int f = 0; f < hb.fpad1; ++f) {
                const u32 on = hb.offn[t * hb.fpad1 + f], ob = hb.off1[t * hb.fpad1 + f];
                const u32 os = hb.offs3[t * hb.fpad1 + f];
                if (f >= F) { if (on != 2u * g.zero_off || ob != 8u * g.zero_off || os != g.zero_off) { std::printf("bit-plane list padding is not the zero block\n"); std::abort(); } continue; }
                if (on != want[(size_t)f]) { std::printf("nibble offset %d of template %zu differs from the per-modality list\n", f, t); std::abort(); }
                const u32 m = (on / 2u) / g.mod_stride, rel = on / 2u - m * g.mod_stride, label = rel / g.ori_stride;
                const u32 pos = on - 2u * (m * g.mod_stride + label * g.ori_stride);                 // position inside the orientation's T * T memories
                const u32 plane0 = 8u * (m * g.mod_stride + 8u * g.ori_stride + label * g.plane_ori);
                if (os != ((label << 29) | (m * g.mod_stride + pos))) { std::printf("spread offset %d of template %zu is not its nibble offset's orientation and position\n", f, t); std::abort(); }
                if (label > 7 || pos >= (u32)(g.T * g.T) * g.wh || ob != plane0 + pos) { std::printf("bit offset %d of template %zu is not its nibble offset's position in the miss plane\n", f, t); std::abort(); }
            }
        }
        for (int L1 : {1, 3, 8, 9, 10, 38, 64}) {
            std::vector<u32> it, ic; std::vector<int> begin;
            lmh::build_items1(hb, L1, it, ic, begin);
            if ((long long)it.size() != hb.items1_by_L[L1] || begin.size() != nt + 1 || begin.back() != (int)it.size()) { std::printf("items of %d lanes per frame: wrong count\n", L1); std::abort(); }
            const int chunk = 128 * L1 - 31;
            for (size_t t = 0; t < nt; ++t) {
                const int n = begin[t + 1] - begin[t];
                if (n != (hb.scan_P[t] + chunk - 1) / chunk) { std::printf("items of %d lanes per frame: template %zu has %d chunks\n", L1, t, n); std::abort(); }
                for (int k = 0; k < n; ++k)
                    if (it[(size_t)begin[t] + k] != (u32)t || ic[(size_t)begin[t] + k] != (u32)k) { std::printf("items of %d lanes per frame: not template-major\n", L1); std::abort(); }
            }
        }
    }
    lmh::HullTable ht;
    lmh::build_hull_table(bank, cfg.num_modalities, ht);
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const std::string dir = argv[4];
    const int iters = std::atoi(argv[2]);
    std::mt19937 rng((unsigned)std::atoi(argv[3]));
    std::string text, err;
    if (!lmy::read_text_file(argv[1], text, err)) { std::printf("cannot read %s: %s\n", argv[1], err.c_str()); return 2; }
    const lm_config cfg0 = make_cfg(2);
    // ---- r05: the staging copies' non-temporal memcpy against memcpy, every alignment of source and destination, lengths around its 32- /
    // 128-byte steps and its fallback threshold; the bytes before and after the destination stay untouched
    {
        std::vector<unsigned char> src(5000), dst(5200), ref(5200);
        for (size_t i = 0; i < src.size(); ++i) src[i] = (unsigned char)rng();
        const size_t lens[] = {0, 1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 300, 1000, 3840, 4097};
        for (size_t len : lens)
            for (size_t so = 0; so < 40; so += 7)
                for (size_t dof = 0; dof < 70; dof += 9) {
                    std::fill(dst.begin(), dst.end(), (unsigned char)0xAB); std::fill(ref.begin(), ref.end(), (unsigned char)0xAB);
                    lmh::copy_stream(dst.data() + 64 + dof, src.data() + so, len);
                    std::memcpy(ref.data() + 64 + dof, src.data() + so, len);
                    lmh::copy_stream_fence();
                    if (dst != ref) { std::printf("copy_stream differs from memcpy (len %zu, src +%zu, dst +%zu)\n", len, so, dof); return 1; }
                }
    }
    // ---- the shifted staging copy (lm_stage_rows and the shifted uploads of pageable frames): lmh::stage_rows_shifted and lmh::shift_rect against a
    // per-pixel translation with zeros shifted in.  The staging buffer (h * row_bytes, 0xAA before the call) and the source ((h - 1) * stride +
    // row_bytes) are heap blocks of their own with exactly the bytes the contract names: a byte read or written outside either is a report.
    // 700 pixels of 3 bytes: a run long enough for copy_stream's non-temporal path.
    long staged = 0;
    {
        std::mt19937 prng(77);      // (its own generator: the mutants below keep theirs)
        for (int w : {1, 2, 7, 33, 700})
            for (int h : {1, 3, 8})
                for (int px : {2, 3})
                    for (size_t gap : {(size_t)0, (size_t)5}) {
                        const size_t row_bytes = (size_t)w * px, stride = row_bytes + gap, src_bytes = (size_t)(h - 1) * stride + row_bytes;
                        std::unique_ptr<u8[]> src(new u8[src_bytes]), stg(new u8[(size_t)h * row_bytes]);
                        for (size_t i = 0; i < src_bytes; ++i) src[i] = (u8)(1 + prng() % 255);      // (never 0: a shifted-in zero is no source byte)
                        std::vector<int> oxs;
                        if (w == 700) oxs = {-700, -699, -13, -1, 0, 1, 7, 699, 700};
                        else for (int o = -w; o <= w; ++o) oxs.push_back(o);
                        for (int ox : oxs)
                            for (int oy = -h; oy <= h; ++oy) {
                                const lmh::ShiftRect q = lmh::shift_rect(w, h, ox, oy);
                                for (int x = 0; x < w; ++x)
                                    if ((x >= q.x0 && x < q.x1) != (x - ox >= 0 && x - ox < w)) { std::printf("shift_rect(%d, %d, %d, %d): column %d\n", w, h, ox, oy, x); return 1; }
                                for (int y = 0; y < h; ++y)
                                    if ((y >= q.y0 && y < q.y1) != (y - oy >= 0 && y - oy < h)) { std::printf("shift_rect(%d, %d, %d, %d): row %d\n", w, h, ox, oy, y); return 1; }
                                for (int pieces : {1, 3}) {
                                    std::memset(stg.get(), 0xAA, (size_t)h * row_bytes);
                                    if (pieces == 1) lmh::stage_rows_shifted(stg.get(), src.get(), stride, w, h, px, ox, oy, 0, h);
                                    else {      // three disjoint row ranges (some empty for small h), not in order
                                        const int a = h / 3, b = (2 * h + 2) / 3;
                                        lmh::stage_rows_shifted(stg.get(), src.get(), stride, w, h, px, ox, oy, b, h);
                                        lmh::stage_rows_shifted(stg.get(), src.get(), stride, w, h, px, ox, oy, 0, a);
                                        lmh::stage_rows_shifted(stg.get(), src.get(), stride, w, h, px, ox, oy, a, b);
                                    }
                                    for (int y = 0; y < h; ++y)
                                        for (int x = 0; x < w; ++x)
                                            for (int k = 0; k < px; ++k) {
                                                const int sx = x - ox, sy = y - oy;
                                                const u8 want = (sx >= 0 && sx < w && sy >= 0 && sy < h) ? src[(size_t)sy * stride + (size_t)sx * px + k] : (u8)0;
                                                if (stg[(size_t)y * row_bytes + (size_t)x * px + k] != want) {
                                                    std::printf("stage_rows_shifted differs from the per-pixel translation (%d x %d, %d bytes per pixel, stride +%zu, shift %d %d, %d pieces) at (%d, %d)\n",
                                                                w, h, px, gap, ox, oy, pieces, x, y);
                                                    return 1;
                                                }
                                            }
                                    ++staged;
                                }
                            }
                    }
    }
    // ---- the valid file: parse, load, digest, write, re-load, bank file round trip
    lmh::Bank good;
    {
        lm_config cfg = cfg0;
        lmy::Node root;
        if (!lmy::parse(text, root, err) || !lmy::load_templates_yaml(good, cfg, argv[1], err)) { std::printf("valid file rejected: %s\n", err.c_str()); return 1; }
        digest(good, cfg);
        const std::string y = dir + "/rt.yml.gz", b = dir + "/rt.bank";
        lmh::Bank again, again2;
        if (!lmy::save_templates_yaml(good, cfg, y.c_str(), err) || !lmy::load_templates_yaml(again, cfg, y.c_str(), err)) { std::printf("yaml round trip: %s\n", err.c_str()); return 1; }
        if (!lmh::save_bank(good, cfg, b.c_str(), err) || !lmh::load_bank(again2, cfg, b.c_str(), err)) { std::printf("bank round trip: %s\n", err.c_str()); return 1; }
        if (again.classes.size() != good.classes.size() || again2.classes.size() != good.classes.size()) { std::printf("round trip lost classes\n"); return 1; }
    }
    std::string bank_bytes;
    { std::ifstream f(dir + "/rt.bank", std::ios::binary); bank_bytes.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()); }
    const char* absurd[] = {"4294967296", "-1", "99999999999999999999", "1e309", "nan", "0x7fffffff", "-2147483648", "[", "]", "{", ":", "- ", "!!opencv-matrix", "\"", "   ", "\t"};
    auto mutate = [&](std::string s) {
        const int n = 1 + (int)(rng() % 4);
        for (int k = 0; k < n && !s.empty(); ++k) {
            const size_t at = rng() % s.size();
            switch (rng() % 7) {
                case 0: s.resize(at); break;                                                     // truncate
                case 1: s[at] = (char)(rng() & 0xFF); break;                                     // flip a byte
                case 2: s.erase(at, std::min<size_t>(1 + rng() % 200, s.size() - at)); break;    // delete a span
                case 3: s.insert(at, s.substr(at, std::min<size_t>(1 + rng() % 300, s.size() - at))); break;   // duplicate a span
                case 4: { const char* a = absurd[rng() % (sizeof(absurd) / sizeof(*absurd))]; s.insert(at, a); break; }
                case 5: { size_t e = at; while (e < s.size() && (std::isdigit((unsigned char)s[e]) || s[e] == '-')) ++e;   // replace a number
                          if (e > at) s.replace(at, e - at, absurd[rng() % 7]); break; }
                default: { size_t e = s.find('\n', at); if (e != std::string::npos) s.erase(at, e - at); break; }   // cut a line short
            }
        }
        return s;
    };
    long accepted = 0, rejected = 0, bank_accepted = 0;
    for (int it = 0; it < iters; ++it) {
        // YAML mutant through the parser and the template loader
        const std::string m = mutate(text), p = dir + "/m.yml";
        { std::ofstream f(p, std::ios::binary); f.write(m.data(), (std::streamsize)m.size()); }
        lmy::Node root;
        std::string e;
        (void)lmy::parse(m, root, e);
        lmh::Bank bank;
        lm_config cfg = cfg0;
        if (lmy::load_templates_yaml(bank, cfg, p.c_str(), e)) { ++accepted; digest(bank, cfg0); } else ++rejected;
        // bank-file mutant
        if ((it & 3) == 0) {
            const std::string bm = mutate(bank_bytes), bp = dir + "/m.bank";
            { std::ofstream f(bp, std::ios::binary); f.write(bm.data(), (std::streamsize)bm.size()); }
            lmh::Bank bb;
            if (lmh::load_bank(bb, cfg0, bp.c_str(), e)) { ++bank_accepted; digest(bb, cfg0); }
        }
    }
    // ---- pathological shapes: deep nesting (recursion depth), one enormous line, a sea of dashes
    {
        std::vector<std::string> evil;
        evil.push_back("%YAML:1.0\n---\nT: " + std::string(200000, '[') + "\n");
        evil.push_back("%YAML:1.0\n---\nT: [ " + std::string(200000, '1') + " ]\n");
        std::string deep = "%YAML:1.0\n---\n";
        for (int i = 0; i < 20000; ++i) deep += std::string((size_t)i, ' ') + "a:\n";
        evil.push_back(deep);
        std::string dashes = "%YAML:1.0\n---\nclasses:\n";
        for (int i = 0; i < 20000; ++i) dashes += std::string((size_t)(3 * (i % 50 + 1)), ' ') + "-\n";
        evil.push_back(dashes);
        for (const std::string& m : evil) {
            lmy::Node root;
            std::string e;
            (void)lmy::parse(m, root, e);
        }
    }
    // ---- feature extraction on random quantised images (lm_extract.cpp)
    for (int it = 0; it < 20; ++it) {
        lm_config cfg = make_cfg(1 + (int)(rng() % 2));
        cfg.width = 64 + 16 * (int)(rng() % 4); cfg.height = 48 + 16 * (int)(rng() % 4);
        std::vector<lmh::ExtractLevel> lv(2);
        for (int l = 0; l < 2; ++l) {
            lv[l].w = cfg.width >> l; lv[l].h = cfg.height >> l;
            const size_t px = (size_t)lv[l].w * lv[l].h;
            lv[l].color_q.resize(px); lv[l].color_mag.resize(px);
            if (cfg.num_modalities == 2) lv[l].depth_q.resize(px);
            if (it & 1) lv[l].mask.assign(px, 0);
            for (size_t i = 0; i < px; ++i) {
                lv[l].color_q[i] = (rng() % 3) ? (u8)(1u << (rng() % 8)) : 0;
                lv[l].color_mag[i] = (float)(rng() % 20000);
                if (cfg.num_modalities == 2) lv[l].depth_q[i] = (rng() % 4) ? (u8)(1u << (rng() % 8)) : 0;
                if (it & 1) lv[l].mask[i] = ((i % lv[l].w) > 5 && (i % lv[l].w) < (size_t)lv[l].w - 6 && i / lv[l].w > 4) ? 255 : 0;
            }
        }
        lmh::TemplatePyramid tp;
        if (lmh::extract_pyramid(lv, cfg, tp)) (void)lmh::crop_templates(tp);
    }
    std::printf("OK yaml mutants accepted %ld rejected %ld, bank mutants accepted %ld, shifted staging cases %ld\n", accepted, rejected, bank_accepted, staged);
    return 0;
}
