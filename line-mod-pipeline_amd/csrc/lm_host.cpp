// lm_host.cpp -- host-only parts of liblinemod_hip.so (see lm_host.h).
#include "lm_host.h"
#if defined(__x86_64__)
#include <immintrin.h>
#endif

#include <algorithm>
#include <atomic>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace lmh {

int Bank::find(const std::string& id) const {
    for (size_t i = 0; i < classes.size(); ++i)
        if (classes[i].id == id) return (int)i;
    return -1;
}

int Bank::add_pyramid(const std::string& id, TemplatePyramid&& tp) {
    int ci = find(id);
    if (ci < 0) { classes.push_back(ClassEntry{id, {}}); ci = (int)classes.size() - 1; }
    classes[ci].pyramids.push_back(std::move(tp));
    return (int)classes[ci].pyramids.size() - 1;
}

bool check_template_pyramid(const TemplatePyramid& tp, int levels, int modalities, std::string& err) {
    if (levels < 1 || modalities < 1 || tp.size() != (size_t)levels * (size_t)modalities) { err = "a pyramid needs levels x modalities templates"; return false; }
    for (int l = 0; l < levels; ++l) {
        size_t nf = 0;
        for (int m = 0; m < modalities; ++m) {
            const Template& t = tp[(size_t)l * modalities + m];
            if (t.pyramid_level != l) { err = "templates must be ordered [level*M + modality]"; return false; }
            if (t.width < 0 || t.height < 0 || t.width > 32767 || t.height > 32767) { err = "template size outside 0..32767"; return false; }
            if (t.features.size() > LM_MAX_FEATURES) { err = "template with more than 63 features (upstream CV_Assert(features.size() <= 63))"; return false; }
            for (const lm_feature& ft : t.features) {
                if (ft.label < 0 || ft.label > 7) { err = "feature label outside 0..7"; return false; }
                if (ft.x < 0 || ft.y < 0 || ft.x > 32767 || ft.y > 32767) { err = "feature coordinate outside 0..32767"; return false; }
            }
            nf += t.features.size();
        }
        if (nf == 0) { err = "template without features at a pyramid level (similarity would divide by zero)"; return false; }
    }
    return true;
}

bool check_modality_params(const lm_config& c, std::string& err) {
    auto fin = [](float v) { return v == v && v >= 0.0f && v < 1e18f; };
    if (!fin(c.weak_threshold) || !fin(c.strong_threshold)) { err = "ColorGradient thresholds must be finite and >= 0"; return false; }
    if (c.num_features < 1 || c.num_features > LM_MAX_FEATURES) { err = "ColorGradient num_features must be in 1..63"; return false; }
    if (c.num_modalities >= 2) {
        if (c.distance_threshold < 0 || c.difference_threshold < 0) { err = "DepthNormal thresholds must be >= 0"; return false; }
        if (c.depth_num_features < 1 || c.depth_num_features > LM_MAX_FEATURES) { err = "DepthNormal num_features must be in 1..63"; return false; }
        if (c.extract_threshold < 0) { err = "DepthNormal extract_threshold must be >= 0"; return false; }
    }
    return true;
}

int Bank::add_class(const std::string& id, int n_templates, const lm_template_desc* descs, const lm_feature* features,
                    int levels, int modalities, std::string& err) {
    const int per = levels * modalities;
    // validate first so a bad call leaves the bank untouched
    size_t fo = 0;
    for (int t = 0; t < n_templates; ++t)
        for (int k = 0; k < per; ++k) {
            const lm_template_desc& ds = descs[(size_t)t * per + k];
            if (ds.num_features < 0 || ds.num_features > LM_MAX_FEATURES) {
                err = "template with more than 63 features (upstream CV_Assert(features.size() <= 63))";
                return -1;
            }
            if (ds.pyramid_level != k / modalities) { err = "template descs must be ordered [level*M + modality]"; return -1; }
            if (ds.width < 0 || ds.height < 0 || ds.width > 32767 || ds.height > 32767) { err = "template size outside 0..32767"; return -1; }
            for (int f = 0; f < ds.num_features; ++f) {
                const lm_feature& ft = features[fo + f];
                if (ft.label < 0 || ft.label > 7) { err = "feature label outside 0..7"; return -1; }
                if (ft.x < 0 || ft.y < 0 || ft.x > 32767 || ft.y > 32767) { err = "feature coordinate outside 0..32767"; return -1; }
            }
            fo += ds.num_features;
        }
    for (int t = 0; t < n_templates; ++t)
        for (int l = 0; l < levels; ++l) {
            int nf = 0;
            for (int m = 0; m < modalities; ++m) nf += descs[(size_t)t * per + l * modalities + m].num_features;
            if (nf == 0) { err = "template without features at a pyramid level (similarity would divide by zero)"; return -1; }
        }
    int ci = find(id);
    if (ci < 0) { classes.push_back(ClassEntry{id, {}}); ci = (int)classes.size() - 1; }
    fo = 0;
    for (int t = 0; t < n_templates; ++t) {
        TemplatePyramid tp(per);
        for (int k = 0; k < per; ++k) {
            const lm_template_desc& ds = descs[(size_t)t * per + k];
            tp[k].width = ds.width; tp[k].height = ds.height; tp[k].pyramid_level = ds.pyramid_level;
            tp[k].features.assign(features + fo, features + fo + ds.num_features);
            fo += ds.num_features;
        }
        classes[ci].pyramids.push_back(std::move(tp));
    }
    return ci;
}

// ------------------------------------------------------------------------------------------------
// Host bank -> device bank of this shard.
//   scan (lowest level, upstream similarity()):  per (template, modality) a list of byte offsets
//     off = m*mod_stride + label*ori_stride + ((y%T)*T + x%T)*W*H + (y/T)*W + x/T
//   into the level arena, padded to `fpad` with offsets of the arena's zero block;
//     P = span_y*W + span_x + 1 = template_positions.
//   refine (levels above the lowest, upstream similarityLocal()): the same offset for the
//     unshifted feature plus (x, y) for the bounds test after the patch offset is applied.
// ------------------------------------------------------------------------------------------------
void schedule_lds_lists(DeviceBankHost& out);
bool build_device_bank(const Bank& bank, const lm_config& cfg, const LmLevelGeom* geom, DeviceBankHost& out,
                       int scan_list_order, std::string& err) {
    const int M = cfg.num_modalities, L = cfg.pyramid_levels;
    out = DeviceBankHost();
    const LmLevelGeom& gl = geom[L - 1];
    int maxf = 1;
    for (const ClassEntry& c : bank.classes)
        for (const TemplatePyramid& tp : c.pyramids)
            for (int m = 0; m < M; ++m) maxf = std::max(maxf, (int)tp[(size_t)(L - 1) * M + m].features.size());
    // byte scan: lists padded to LM_SCAN_FPAD; nibble scan (k_scan4): loops to the pair's own feature count, offsets in nibbles
    const int fq = gl.nibble ? 1 : LM_SCAN_FPAD;
    const u32 osc = gl.nibble ? 2u : 1u;
    out.fpad = (maxf + fq - 1) / fq * fq;
    const int nc = (int)bank.classes.size();
    out.class_item_lo.assign(nc, 0); out.class_item_hi.assign(nc, 0);
    out.class_t_lo.assign(nc, 0); out.class_t_hi.assign(nc, 0);
    out.class_alg_bytes.assign(nc, 0.0);
    out.class_load_bytes.assign(nc, 0.0);
    const bool planes = gl.nibble && gl.plane_ori != 0;
    if (planes) out.fpad1 = (std::min(M * maxf, 2 * LM_MAX_FEATURES) + 7) / 8 * 8;       // (k_scan1_exact reads whole batches of eight: the padding is the zero block)
    // r06: the LDS image of a frame's planes (k_scanl) -- [modality][orientation][pb bytes], pb = T*T*wh / 8, nothing between the planes
    const u32 ttwh = (u32)gl.T * (u32)gl.T * gl.wh, pb = ttwh / 8u;
    out.lds_ok = lds_image_fits(gl, M);
    // a list entry's bit offset from its nibble offset: the planes of a modality follow its 8 response memories
    auto plane_bit_off = [&](u32 noff) {
        const u32 base = noff / 2u, m = base / gl.mod_stride, label = (base - m * gl.mod_stride) / gl.ori_stride;
        const u32 rest = noff - 2u * (m * gl.mod_stride + label * gl.ori_stride);
        return 8u * (m * gl.mod_stride + 8u * gl.ori_stride + label * gl.plane_ori) + rest;
    };
    for (int ci = 0; ci < nc; ++ci) {
        const ClassEntry& c = bank.classes[ci];
        int lo, hi;
        shard_range((int)c.pyramids.size(), cfg.shard_rank, cfg.shard_size, &lo, &hi);
        out.class_t_lo[ci] = (int)out.t_global.size();
        out.class_item_lo[ci] = (int)out.item_t.size();
        // (k_scanl: a class starts a fresh wave item, so that the lanes that meet in one LDS access are the same whichever classes a launch scans;
        // the fillers are "no item")
        if (out.lds_ok) while (out.litem.size() % 64u) out.litem.push_back(0xFFFFFFFFu);
        for (int tid = lo; tid < hi; ++tid) {
            const TemplatePyramid& tp = c.pyramids[tid];
            if ((int)tp.size() != L * M) { err = "template pyramid size mismatch"; return false; }
            const u32 ti = (u32)out.t_global.size();
            out.t_global.push_back(tid);
            out.t_class.push_back(ci);
            // ---- scan level
            const Template& t0 = tp[(size_t)(L - 1) * M];
            int n_total = 0, cnt_packed = 0;
            int P = 0;
            double fcount = 0;
            for (int m = 0; m < M; ++m) {
                const Template& t = tp[(size_t)(L - 1) * M + m];
                n_total += (int)t.features.size();
                // upstream computes the span per modality from that modality's own template size; all
                // templates of one pyramid level share width/height after cropTemplates, so use each
                // modality's own value and require them equal.
                if (t.width != t0.width || t.height != t0.height) { err = "modalities of one pyramid level must share width/height"; return false; }
                int wf = (t.width - 1) / gl.T + 1, hf = (t.height - 1) / gl.T + 1;
                const int span_x = gl.W - wf, span_y = gl.H - hf;
                const long long P64 = (long long)span_y * gl.W + span_x + 1;
                P = (int)std::min<long long>(std::max<long long>(P64, 0), (long long)gl.wh);
                int k = 0;
                const size_t list_begin = out.scan_off.size();
                for (const lm_feature& f : t.features) {
                    if (f.x < 0 || f.x >= gl.w || f.y < 0 || f.y >= gl.h) continue;  // similarity(): "discard feature if out of bounds"
                    u32 off = osc * ((u32)m * gl.mod_stride + (u32)f.label * gl.ori_stride) +
                              (u32)((f.y % gl.T) * gl.T + (f.x % gl.T)) * gl.wh + (u32)(f.y / gl.T) * gl.W + (u32)(f.x / gl.T);
                    out.scan_off.push_back(off);
                    ++k;
                }
                fcount += k;
                cnt_packed |= k << (8 + 8 * m);
                // the sum is order-independent: ascending offsets make the waves resident on one CU (they start
                // together and step through their lists in step) read from the same few linear memories at a
                // time, so part of the traffic is served by the CU's L1 instead of L2
                std::sort(out.scan_off.begin() + (ptrdiff_t)list_begin, out.scan_off.end());
                {
                    // r04: the ORDER of a list decides how soon the scan's exact pruning gives up on a work item (the sums do not depend
                    // on it).  Sorted by offset (0) a list starts with ALL its features of orientation 0, whose responses rise and fall
                    // together over the frame.  3 (default): greedy farthest-point order in (x, y, orientation) -- every next feature is the
                    // one farthest from all chosen so far, an orientation step counting like 4 pixels -- so the first features sample the
                    // template's whole extent and all its orientations.  Measured, share of the feature loads the pruned scan makes /
                    // scan launch (profiles/r04_ab_experiments.log): config 2 49.7 % / 167 us (0), 48.2 % / 164 (1: round-robin over the
                    // orientations), 50.5 % (2: descending offsets), 46.3 % / 158.5 (3); config 3 42.7 % / 409 -> 39.8 % / 392.
                    const int feat_order = scan_list_order;
                    if (feat_order == 2) std::reverse(out.scan_off.begin() + (ptrdiff_t)list_begin, out.scan_off.end());
                    if (feat_order == 1) {
                        std::vector<std::vector<u32>> by_label(8);
                        for (size_t q = list_begin; q < out.scan_off.size(); ++q) {
                            const u32 rel = out.scan_off[q] / osc - (u32)m * gl.mod_stride;
                            by_label[std::min<u32>(rel / gl.ori_stride, 7u)].push_back(out.scan_off[q]);
                        }
                        size_t q = list_begin;
                        for (size_t r = 0; q < out.scan_off.size(); ++r)
                            for (int lb = 0; lb < 8; ++lb) if (r < by_label[lb].size()) out.scan_off[q++] = by_label[lb][r];
                    }
                    if (feat_order == 3) {
                        struct FP { u32 off; int x, y, lab; };
                        std::vector<FP> fp;
                        for (const lm_feature& f : t.features) {
                            if (f.x < 0 || f.x >= gl.w || f.y < 0 || f.y >= gl.h) continue;
                            const u32 off = osc * ((u32)m * gl.mod_stride + (u32)f.label * gl.ori_stride) +
                                            (u32)((f.y % gl.T) * gl.T + (f.x % gl.T)) * gl.wh + (u32)(f.y / gl.T) * gl.W + (u32)(f.x / gl.T);
                            fp.push_back(FP{off, f.x, f.y, f.label});
                        }
                        std::vector<long> best(fp.size(), (long)1 << 40);
                        std::vector<char> used(fp.size(), 0);
                        size_t cur = 0;
                        for (size_t q = 1; q < fp.size(); ++q) if (fp[q].off < fp[cur].off) cur = q;     // starts at the smallest offset
                        for (size_t r = 0; r < fp.size(); ++r) {
                            out.scan_off[list_begin + r] = fp[cur].off;
                            used[cur] = 1;
                            size_t nxt = cur; long far = -1;
                            for (size_t q = 0; q < fp.size(); ++q) {
                                if (used[q]) continue;
                                const int dl = std::min((fp[q].lab - fp[cur].lab) & 7, (fp[cur].lab - fp[q].lab) & 7);
                                const long dd = (long)(fp[q].x - fp[cur].x) * (fp[q].x - fp[cur].x) + (long)(fp[q].y - fp[cur].y) * (fp[q].y - fp[cur].y) + 16L * dl * dl;
                                best[q] = std::min(best[q], dd);
                                if (best[q] > far || (best[q] == far && fp[q].off < fp[nxt].off)) { far = best[q]; nxt = q; }
                            }
                            cur = nxt;
                        }
                    }
                }
                for (; k < out.fpad; ++k) out.scan_off.push_back(osc * gl.zero_off);
            }
            if (planes) {
                const size_t b1 = out.off1.size();
                for (int m = 0; m < M; ++m) {
                    const int k = (cnt_packed >> (8 + 8 * m)) & 0xFF;
                    const size_t lb = ((size_t)ti * M + m) * out.fpad;
                    for (int q = 0; q < k; ++q) {
                        const u32 noff = out.scan_off[lb + q];
                        out.offn.push_back(noff); out.off1.push_back(plane_bit_off(noff));
                        const u32 base = noff / 2u, mm = base / gl.mod_stride, label = (base - mm * gl.mod_stride) / gl.ori_stride;
                        out.offs3.push_back((label << 29) | (mm * gl.mod_stride + (noff - 2u * (mm * gl.mod_stride + label * gl.ori_stride))));
                    }
                }
                if (out.lds_ok) {
                    for (size_t q = b1; q < out.off1.size(); ++q) {
                        const u32 e3 = out.offs3[q], label = e3 >> 29, so = e3 & 0x1FFFFFFFu, mm = so / gl.mod_stride, rest = so - mm * gl.mod_stride;     // rest = memory * wh + cell
                        const u32 bit = 8u * (mm * 8u + label) * pb + rest;
                        out.offl.push_back((((bit >> 5) << 2) << 8) | (bit & 31u));
                        out.offsl.push_back((label << 29) | (mm * ttwh + rest));
                    }
                    // (padding: the image's zero block, right behind the planes; the second stage stops at a template's own feature count)
                    while (out.offl.size() < b1 + (size_t)out.fpad1) { out.offl.push_back(((u32)M * ttwh) << 8); out.offsl.push_back(0u); }
                    out.lbegin.push_back((int)out.litem.size());
                    for (int un = 0; un * 128 < P; ++un) out.litem.push_back((ti << 8) | (u32)un);
                }
                // (padding: the zero block through orientation 0 -- response 0 whatever the table, it maps an empty spread byte to 0)
                while (out.off1.size() < b1 + (size_t)out.fpad1) { out.offn.push_back(2u * gl.zero_off); out.off1.push_back(8u * gl.zero_off); out.offs3.push_back(gl.zero_off); }
                for (int L1 = 1; L1 <= 64; ++L1) out.items1_by_L[L1] += (P + (128 * L1 - 31) - 1) / (128 * L1 - 31);
            }
            const int chunk = gl.nibble ? LM_SCAN4_CHUNK : LM_SCAN_CHUNK;
            out.scan_P.push_back(P);
            out.scan_n.push_back(n_total | cnt_packed);   // n (bits 0-7) | in-bounds features of modality 0 / 1 (bits 8-15 / 16-23)
            out.class_alg_bytes[ci] += fcount * (double)P;
            // what the scan's vector loads request: per feature and work item one half-wave x 16 B (nibble
            // layout) or one wave x 16 B (byte layout)
            out.class_load_bytes[ci] += fcount * (double)((P + chunk - 1) / chunk) * (gl.nibble ? 512.0 : 1024.0);
            for (int ch = 0; ch * chunk < P; ++ch) { out.item_t.push_back(ti); out.item_chunk.push_back((u32)ch); }
            // ---- refinement levels
            for (int l = 0; l + 1 < L; ++l) {
                const LmLevelGeom& g = geom[l];
                LmRefMeta mt;
                std::memset(&mt, 0, sizeof(mt));
                mt.width = tp[(size_t)l * M].width;
                mt.height = tp[(size_t)l * M].height;
                for (int m = 0; m < M; ++m) {
                    const Template& t = tp[(size_t)l * M + m];
                    mt.nfeat_total += (int)t.features.size();
                    mt.start[m] = (u32)out.ref_feat[l].size();
                    mt.count[m] = (u32)t.features.size();
                    for (const lm_feature& f : t.features) {
                        LmRefFeat rf;
                        // spread arena: [modality][memory (y%T)*T + x%T][(y/T)*W + x/T]; label rides in the top bits
                        rf.off = ((u32)m * g.mod_stride + (u32)((f.y % g.T) * g.T + (f.x % g.T)) * g.wh +
                                  (u32)(f.y / g.T) * g.W + (u32)(f.x / g.T)) |
                                 ((u32)f.label << 29);
                        if ((u64)m * g.mod_stride + (u64)((f.y % g.T) * g.T + (f.x % g.T)) * g.wh + (u64)(f.y / g.T) * g.W +
                                (u64)(f.x / g.T) >= (1ull << 29)) { err = "feature too far outside the frame"; return false; }
                        rf.x = (int16_t)f.x; rf.y = (int16_t)f.y;
                        out.ref_feat[l].push_back(rf);
                    }
                }
                out.ref_meta[l].push_back(mt);
            }
        }
        out.class_t_hi[ci] = (int)out.t_global.size();
        out.class_item_hi[ci] = (int)out.item_t.size();
    }
    if (out.lds_ok) {
        out.lbegin.push_back((int)out.litem.size());
        if (out.t_global.size() >= (1u << (32 - LM_SCANL_POS_BITS)) || out.litem.empty()) out.lds_ok = false;     // (the survivor entry's template field)
    }
    if (out.lds_ok) {
        schedule_lds_lists(out);
        out.lrec.assign(out.litem.size() * 4u, 0u);
        for (size_t i = 0; i < out.litem.size(); ++i) {
            const u32 it = out.litem[i];
            out.lrec[4 * i] = it;
            if (it != 0xFFFFFFFFu) { out.lrec[4 * i + 1] = (u32)out.scan_n[it >> 8]; out.lrec[4 * i + 2] = (u32)out.scan_P[it >> 8]; }
        }
    }
    return true;
}

// r06: the ORDER of k_scanl's lists against LDS bank conflicts.  A lane reads the dwords D + 4 u + q of a feature's plane (D: the feature's first dword,
// u: the lane's unit, q = 0..4), one ds_read_b32-sized access per q; the hardware serves 32 lanes per cycle from 32 banks.  The lanes of ONE template hit
// the eight banks = (D + q) mod 4; two templates of a 32-lane group whose features have the same D mod 4 at the same step collide on all of them
// (measured: 25 of 109 us per 96-frame launch of config 2 are conflict cycles; four templates at random residues serve an access in 2.1 cycles instead of
// 1).  The sums do not depend on the order of a list, so every template's list is permuted -- greedily, first fit in its own (farthest-point) order -- such
// that at each step its residue differs from those of the templates it shares a 32-lane group with.  Only the order of `offl` changes.
void schedule_lds_lists(DeviceBankHost& out) {
    const size_t nt = out.t_global.size();
    const int fp = out.fpad1;
    auto residue = [](u32 e) { return (int)(((e >> 8) >> 2) & 3u); };
    std::vector<u32> tmp((size_t)fp);
    std::vector<char> used((size_t)fp);
    for (size_t t = 0; t < nt; ++t) {
        const int lb = out.lbegin[t], le = out.lbegin[t + 1];
        // lane items of template t: [lb, le) minus trailing fillers; none: nothing to schedule
        int last = le;
        while (last > lb && out.litem[(size_t)last - 1] == 0xFFFFFFFFu) --last;
        if (last <= lb) continue;
        const int g_first = lb / 32;
        // neighbours: earlier templates with a lane in one of this template's groups (they are scheduled already)
        std::vector<size_t> nb;
        for (size_t p = t; p-- > 0 && nb.size() < 8;) {
            int pl = out.lbegin[p + 1];
            while (pl > out.lbegin[p] && out.litem[(size_t)pl - 1] == 0xFFFFFFFFu) --pl;
            if (pl <= out.lbegin[p]) continue;
            if ((pl - 1) / 32 < g_first) break;
            nb.push_back(p);
        }
        if (nb.empty()) continue;
        u32* list = out.offl.data() + t * (size_t)fp;
        // the list's real entries = the template's in-bounds features (the padding, entries of the zero block, stays at the end)
        const int cnt = out.scan_n[t];
        const int nreal = std::min(fp, ((cnt >> 8) & 0xFF) + ((cnt >> 16) & 0xFF));
        std::fill(used.begin(), used.end(), 0);
        for (int k = 0; k < nreal; ++k) {
            bool taken[4] = {false, false, false, false};
            for (size_t p : nb) taken[residue(out.offl[p * (size_t)fp + (size_t)k])] = true;
            int pick = -1, first = -1;
            for (int q = 0; q < nreal; ++q) {
                if (used[(size_t)q]) continue;
                if (first < 0) first = q;
                if (!taken[residue(list[q])]) { pick = q; break; }
            }
            if (pick < 0) pick = first;
            used[(size_t)pick] = 1;
            tmp[(size_t)k] = list[pick];
        }
        for (int k = 0; k < nreal; ++k) list[k] = tmp[(size_t)k];
    }
}

void build_items1(const DeviceBankHost& hb, int L, std::vector<u32>& item_t, std::vector<u32>& item_chunk, std::vector<int>& begin) {
    const int chunk = 128 * L - 31;
    item_t.clear(); item_chunk.clear(); begin.clear();
    for (size_t t = 0; t < hb.scan_P.size(); ++t) {
        begin.push_back((int)item_t.size());
        for (int ch = 0; ch * chunk < hb.scan_P[t]; ++ch) { item_t.push_back((u32)t); item_chunk.push_back((u32)ch); }
    }
    begin.push_back((int)item_t.size());
}

void build_hull_table(const Bank& bank, int M, HullTable& out) {
    out = HullTable();
    struct P { int x, y; };
    std::vector<P> p, hull;
    for (const ClassEntry& c : bank.classes) {
        out.class_base.push_back((u32)out.hull_off.size());
        for (const TemplatePyramid& tp : c.pyramids) {
            out.hull_off.push_back((u32)(out.hull_xy.size() / 2));
            p.clear();
            for (int m = 0; m < M && m < (int)tp.size(); ++m)          // tp[m], m < M: the level-0 templates
                for (const lm_feature& f : tp[(size_t)m].features) p.push_back(P{f.x, f.y});
            std::sort(p.begin(), p.end(), [](const P& a, const P& b) { return a.x < b.x || (a.x == b.x && a.y < b.y); });
            p.erase(std::unique(p.begin(), p.end(), [](const P& a, const P& b) { return a.x == b.x && a.y == b.y; }), p.end());
            if (p.size() >= 3) {
                auto crs = [](const P& o, const P& a, const P& b) { return (long long)(a.x - o.x) * (b.y - o.y) - (long long)(a.y - o.y) * (b.x - o.x); };
                hull.assign(2 * p.size(), P{0, 0});
                size_t k = 0;
                for (size_t i = 0; i < p.size(); ++i) {
                    while (k >= 2 && crs(hull[k - 2], hull[k - 1], p[i]) <= 0) --k;
                    hull[k++] = p[i];
                }
                for (size_t i = p.size() - 1, t = k + 1; i > 0; --i) {
                    while (k >= t && crs(hull[k - 2], hull[k - 1], p[i - 1]) <= 0) --k;
                    hull[k++] = p[i - 1];
                }
                hull.resize(k - 1);
            } else {
                hull = p;
            }
            for (const P& q : hull) { out.hull_xy.push_back((int16_t)q.x); out.hull_xy.push_back((int16_t)q.y); }
        }
    }
    out.hull_off.push_back((u32)(out.hull_xy.size() / 2));
    if (out.class_base.empty()) out.class_base.push_back(0);
}

// SIMILARITY_LUT default = the table cv::linemod ships (layout [ori][lo nibble 16 | hi nibble 16],
// entry = max over the nibble's set bits of the single-bit score).  Rows 3-7 are circular in the 8 orientation
// bins, rows 0-2 are not (orientation 0 scores 0 against bits 5-7): an upstream quirk that is part of the
// reference's behaviour, so it is the default here; lm_set_similarity_lut replaces it.
void default_similarity_lut(u8 lut[256]) {
    static const u8 kUpstream[256] = {
        0, 4, 3, 4, 2, 4, 3, 4, 1, 4, 3, 4, 2, 4, 3, 4,  0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        0, 3, 4, 4, 3, 3, 4, 4, 2, 3, 4, 4, 3, 3, 4, 4,  0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1,
        0, 2, 3, 3, 4, 4, 4, 4, 3, 3, 3, 3, 4, 4, 4, 4,  0, 2, 1, 2, 0, 2, 1, 2, 0, 2, 1, 2, 0, 2, 1, 2,
        0, 1, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4,  0, 3, 2, 3, 1, 3, 2, 3, 0, 3, 2, 3, 1, 3, 2, 3,
        0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3,  0, 4, 3, 4, 2, 4, 3, 4, 1, 4, 3, 4, 2, 4, 3, 4,
        0, 1, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2,  0, 3, 4, 4, 3, 3, 4, 4, 2, 3, 4, 4, 3, 3, 4, 4,
        0, 2, 1, 2, 0, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2,  0, 2, 3, 3, 4, 4, 4, 4, 3, 3, 3, 3, 4, 4, 4, 4,
        0, 3, 2, 3, 1, 3, 2, 3, 0, 3, 2, 3, 1, 3, 2, 3,  0, 1, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4};
    std::memcpy(lut, kUpstream, 256);
}

// NORMAL_LUT default (our documented rule): azimuth of the cell centre, 8 bins.
void default_normal_lut(u8 lut[8000]) {
    const double PI = 3.14159265358979323846;
    for (int v3 = 0; v3 < 20; ++v3)
        for (int v2 = 0; v2 < 20; ++v2)
            for (int v1 = 0; v1 < 20; ++v1) {
                double nx = (v1 + 0.5 - 10.0) / 10.0, ny = (v2 + 0.5 - 10.0) / 10.0;
                double a = std::atan2(ny, nx);
                if (a < 0) a += 2 * PI;
                int bin = (int)std::floor(a / (PI / 4.0));
                if (bin > 7) bin = 7;
                lut[v3 * 400 + v2 * 20 + v1] = (u8)(1u << bin);
            }
}

bool match_less(const lm_match_t& a, const lm_match_t& b) {
    if (a.similarity != b.similarity) return a.similarity > b.similarity;
    if (a.template_id != b.template_id) return a.template_id < b.template_id;
    if (a.class_idx != b.class_idx) return a.class_idx < b.class_idx;
    if (a.y != b.y) return a.y < b.y;
    return a.x < b.x;
}
bool match_eq(const lm_match_t& a, const lm_match_t& b) {
    return a.x == b.x && a.y == b.y && a.similarity == b.similarity && a.class_idx == b.class_idx;
}
void sort_unique(std::vector<lm_match_t>& v) {
    std::sort(v.begin(), v.end(), match_less);
    v.erase(std::unique(v.begin(), v.end(), match_eq), v.end());
}

// ------------------------------------------------------------------------------------------------
// Bank file: "LMBK0001" | u32 levels | u32 modalities | u32 T[levels] | u32 n_classes |
//   per class { u32 id_len | id bytes | u32 n_templates | descs[n*levels*M] | u32 n_features | features[] }
// little endian, descs/features in the lm_template_desc / lm_feature layouts.
// ------------------------------------------------------------------------------------------------
namespace {
struct File {
    FILE* f;
    explicit File(FILE* fp) : f(fp) {}
    ~File() { if (f) fclose(f); }
};
bool wr(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
}  // namespace

bool save_bank(const Bank& bank, const lm_config& cfg, const char* path, std::string& err) {
    File fh(fopen(path, "wb"));
    if (!fh.f) { err = std::string("cannot open for writing: ") + path; return false; }
    const u32 L = (u32)cfg.pyramid_levels, M = (u32)cfg.num_modalities;
    bool ok = wr(fh.f, "LMBK0001", 8) && wr(fh.f, &L, 4) && wr(fh.f, &M, 4);
    for (u32 l = 0; l < L; ++l) { u32 t = (u32)cfg.T[l]; ok = ok && wr(fh.f, &t, 4); }
    u32 nc = (u32)bank.classes.size();
    ok = ok && wr(fh.f, &nc, 4);
    for (const ClassEntry& c : bank.classes) {
        u32 len = (u32)c.id.size(), nt = (u32)c.pyramids.size();
        ok = ok && wr(fh.f, &len, 4) && wr(fh.f, c.id.data(), len) && wr(fh.f, &nt, 4);
        std::vector<lm_template_desc> descs;
        std::vector<lm_feature> feats;
        for (const TemplatePyramid& tp : c.pyramids)
            for (const Template& t : tp) {
                descs.push_back(lm_template_desc{t.width, t.height, t.pyramid_level, (int32_t)t.features.size()});
                feats.insert(feats.end(), t.features.begin(), t.features.end());
            }
        u32 nf = (u32)feats.size();
        ok = ok && wr(fh.f, descs.data(), descs.size() * sizeof(lm_template_desc)) && wr(fh.f, &nf, 4) &&
             wr(fh.f, feats.data(), feats.size() * sizeof(lm_feature));
    }
    if (!ok) { err = std::string("short write: ") + path; return false; }
    return true;
}

bool load_bank(Bank& bank, const lm_config& cfg, const char* path, std::string& err) {
    File fh(fopen(path, "rb"));
    if (!fh.f) { err = std::string("cannot open: ") + path; return false; }
    char magic[8];
    u32 L = 0, M = 0;
    if (!rd(fh.f, magic, 8) || std::memcmp(magic, "LMBK0001", 8) != 0) { err = "not a linemod bank file"; return false; }
    if (!rd(fh.f, &L, 4) || !rd(fh.f, &M, 4)) { err = "truncated bank file"; return false; }
    if ((int)L != cfg.pyramid_levels || (int)M != cfg.num_modalities) { err = "bank was written for a different detector (levels/modalities)"; return false; }
    for (u32 l = 0; l < L; ++l) {
        u32 t = 0;
        if (!rd(fh.f, &t, 4)) { err = "truncated bank file"; return false; }
        if ((int)t != cfg.T[l]) { err = "bank was written for a different T pyramid"; return false; }
    }
    u32 nc = 0;
    if (!rd(fh.f, &nc, 4)) { err = "truncated bank file"; return false; }
    // counts read from the file size buffers below: none may promise more bytes than the file holds
    long here = std::ftell(fh.f);
    if (here < 0 || std::fseek(fh.f, 0, SEEK_END) != 0) { err = "cannot seek in bank file"; return false; }
    const unsigned long long file_bytes = (unsigned long long)std::ftell(fh.f);
    if (std::fseek(fh.f, here, SEEK_SET) != 0) { err = "cannot seek in bank file"; return false; }
    Bank nb;
    for (u32 c = 0; c < nc; ++c) {
        u32 len = 0, nt = 0, nf = 0;
        if (!rd(fh.f, &len, 4) || len > 4096) { err = "corrupt bank file"; return false; }
        std::string id(len, '\0');
        if (!rd(fh.f, &id[0], len) || !rd(fh.f, &nt, 4)) { err = "truncated bank file"; return false; }
        if ((unsigned long long)nt * L * M * sizeof(lm_template_desc) > file_bytes) { err = "corrupt bank file (template count)"; return false; }
        std::vector<lm_template_desc> descs((size_t)nt * L * M);
        if (!rd(fh.f, descs.data(), descs.size() * sizeof(lm_template_desc)) || !rd(fh.f, &nf, 4)) { err = "truncated bank file"; return false; }
        unsigned long long want = 0;
        for (const auto& ds : descs) want += (unsigned)std::max(ds.num_features, 0);
        if (want != nf || (unsigned long long)nf * sizeof(lm_feature) > file_bytes) { err = "corrupt bank file (feature count)"; return false; }
        std::vector<lm_feature> feats(nf);
        if (!rd(fh.f, feats.data(), feats.size() * sizeof(lm_feature))) { err = "truncated bank file"; return false; }
        if (nb.add_class(id, (int)nt, descs.data(), feats.data(), (int)L, (int)M, err) < 0) return false;
        if (nt == 0 && nb.find(id) < 0) nb.classes.push_back(ClassEntry{id, {}});
    }
    bank = std::move(nb);
    return true;
}

bool lds_image_fits(const LmLevelGeom& g, int M) {
    const u32 ttwh = (u32)g.T * (u32)g.T * g.wh;
    return g.nibble && g.plane_ori && (ttwh % 128u) == 0 && (size_t)M * ttwh <= LM_SCANL_IMAGE_MAX && g.wh <= (1u << LM_SCANL_POS_BITS);
}

// The bit-plane scan k_scan1 issues about as many vector instructions per wave and feature as the nibble scan k_scan4, and a wave of either
// is one work item for a group of frames: 64 / L1 frames of chunks of 128 L1 - 31 positions there, two frames of chunks of 1016 here.  So
// the form with fewer waves wins; L1 is the lane count with the fewest (0: none fits), `waves` their number.
static int fewest_waves(const ScanInputs& in, int nslots, long long* waves = nullptr) {
    if (!in.nibble || !in.planes || !in.fpad1) return 0;
    long long best = -1; int bestL = 0;
    for (int L1 = 1; L1 <= 64; ++L1) {
        const int G1 = 64 / L1;
        // a wave's buffer descriptor starts at its group's first frame: the last frame's arena must end below 2^31 bytes
        if ((size_t)(G1 - 1) * in.frame_stride + in.arena_bytes >= 0x7FFFFFFFull) continue;
        const long long w = in.items1_by_L[L1] * ((nslots + G1 - 1) / G1);
        if (best < 0 || w < best) { best = w; bestL = L1; }
    }
    if (waves) *waves = best;
    return bestL;
}

// k_scan1's lanes per frame by the rules, 0 = not k_scan1.  By cost it needs a margin (its waves stop when the LAST of their frames is out of
// reach, and the survivors' exact sums come on top), whole groups of frames, and a threshold high enough for the miss bound to bite.
static int scan1_lanes(const ScanInputs& in, int nslots) {
    if (in.form == 1) return 0;
    const bool asked = in.form >= 2;      // (3: k_scanl where a frame's planes fit, this kernel where they do not)
    // measured r05 (profiles/r05_ab_experiments.log, three lanes): colour-only config 3 +9 % (the scan launch 389 -> 296 us per 128 frames), but
    // RGB-D config 2 -2 % and config 5 -18 %: with two modalities the exact deficits of k_scan4's pruning stop a work item after 29-46 % of its
    // features, the miss bound after 66-84 %.  By cost = one modality only, and batches only: its three launches (queue reset, k_scan1,
    // k_scan1_exact) cost a single 640 x 480 frame 29 instead of 15 us of scan (the reference's one-frame call: 100 against 89 us per call)
    if (!asked && (!(in.threshold >= in.scan1_min_threshold) || in.M != 1 || nslots < 8)) return 0;
    long long waves = 0;
    const int L1 = fewest_waves(in, nslots, &waves);
    if (L1 == 0 || asked) return L1;
    const long long waves4 = in.items4 * ((nslots + 1) / 2);
    return (waves * 5 > waves4 * 4 || nslots < 64 / L1) ? 0 : L1;
}

// r06, k_scanl's workgroups (shares of the lane items) per frame: a workgroup takes a CU's whole LDS, so the chip runs 256 at a time; each pays a
// fixed price (the two copies of 150 KB, two barriers, the wait for its last wave: about 14 us) plus about 10 us per wave item of its busiest
// wave.  Measured on config 2's workload (tools/probe_scanl_R.py, profiles/r06_ab_experiments.log): the best share count fills ONE round of the
// chip up to 64 frames and two beyond (32 frames: 8 shares, 64: 4, 96: 5, 128: 4); below 4 shares a workgroup's survivors no longer fit its
// LDS queue.  The model below reproduces those choices.  LM_SCANL_R overrides it within the same range.
static int scanl_shares(const ScanInputs& in, int nslots, int n_litems) {
    const int n_w = (n_litems + 63) / 64;
    const int r_max = std::max(1, std::min(32, n_w / 16));        // (every wave of a workgroup gets an item)
    if (in.scanl_R > 0) return std::min(in.scanl_R, r_max);
    const int r_min = std::min(4, r_max);
    int best = r_min; double best_t = -1;
    for (int R = r_min; R <= r_max; ++R) {
        const double x = (double)nslots * R / 256.0, rounds = std::max(1.0, 0.7 * std::ceil(x) + 0.3 * x);
        const double t = rounds * (14.2 + 9.8 * ((n_w + 16 * R - 1) / (16 * R)));
        if (best_t < 0 || t < best_t - 1e-9) { best_t = t; best = R; }
    }
    return best;
}

static bool scanl_available(const ScanInputs& in) {
    return in.bank_built && in.scanl_bank && in.scanl_device && in.form != 1 && in.form != 2;
}

// The miss planes cost the pass that writes them a second set of scattered stores (measured r05: 16.2 -> 24.4 us per 96-frame launch of
// config 2, 70 -> 115 us per 128 frames of config 3): they are written only where a bit-plane scan can run -- by cost for a call of 8+
// frames on a one-modality detector or one k_scanl takes; form 2 always, 1 never.  When this call's own scan is a bit-plane one by the
// rules, the level gets the spread byte INSTEAD of the response memories (the pass is bound by the number of its stores), and its slots
// can only be scanned by a bit-plane form afterwards; form 3 writes it wherever a frame's planes fit LDS, whatever the bank.
Layout plan_layout(const ScanInputs& in, int n) {
    if (in.form == 1 || !in.planes) return Layout::Responses;
    // k_scanl by cost: calls of enough frames to fill the chip with its workgroups, at thresholds at which the miss bound bites
    const bool scanl = scanl_available(in) && in.nibble &&
                       (in.form == 3 || (in.threshold >= in.scan1_min_threshold && n >= in.scanl_min_slots));
    if (in.form == 0 && !scanl && !(in.M == 1 && n >= 8)) return Layout::Responses;
    const bool spread = in.form == 3 ? in.lds_fits : in.form == 0 && in.bank_built && (scanl || scan1_lanes(in, n) > 0);
    return spread ? Layout::SpreadAndPlanes : Layout::ResponsesAndPlanes;
}

ScanPlan plan_scan(const ScanInputs& in, int nslots, unsigned layouts, int n_litems) {
    if (layouts_mixed(layouts)) return {ScanPlan::Mixed, 0};
    if (layouts == layout_bit(Layout::SpreadAndPlanes)) {
        // prepared for a bit-plane scan: k_scanl whenever it can run (by cost from scanl_min_slots frames, whatever the threshold now: calls of
        // fewer frames stay with k_scan1, which such slots can take as well), else k_scan1 with the fewest waves whatever the rules say
        if (scanl_available(in) && n_litems > 0 && !(in.form == 0 && nslots < in.scanl_min_slots))
            return {ScanPlan::ScanL, scanl_shares(in, nslots, n_litems)};
        const int L1 = fewest_waves(in, nslots);
        return L1 ? ScanPlan{ScanPlan::Scan1, L1} : ScanPlan{ScanPlan::NoBitPlaneForm, 0};
    }
    // (k_scan1 only when every frame's pass wrote the planes)
    const int L1 = layouts == layout_bit(Layout::ResponsesAndPlanes) ? scan1_lanes(in, nslots) : 0;
    return L1 ? ScanPlan{ScanPlan::Scan1, L1} : ScanPlan{ScanPlan::Scan4, 0};
}

// ================================================================================================
// The match-stage planner (lm_host.h): one range of classes over nslots frames -> the ordered launches of a11-a15 and the numbers their
// argument structs derive from the call.
// ================================================================================================
const char* match_kernel_name(MatchKernel k) {
    static const char* const names[(int)MatchKernel::Count] = {
        "surv_reset",
        "k_scan<8,true>", "k_scan<4,true>", "k_scan<2,true>", "k_scan<8,false>", "k_scan<4,false>", "k_scan<2,false>",
        "k_scan4<6,true,0>", "k_scan4<6,true,1>", "k_scan4<6,true,2>", "k_scan4<12,true,0>", "k_scan4<12,true,1>", "k_scan4<12,true,2>",
        "k_scan4<3,true,0>", "k_scan4<3,true,1>", "k_scan4<3,true,2>", "k_scan4<6,true,0,true>",
        "k_scan1", "k_scan1_exact", "k_scanl",
        "k_refine_plan", "k_refine<false,false>", "k_refine<false,true>", "k_refine<true,false>", "k_refine<true,true>",
        "k_emit_unrefined", "k_sort_unique", "k_merge_unique",
    };
    return k < MatchKernel::Count ? names[(int)k] : "?";
}

MatchStep& MatchPlan::add(MatchKernel k, u32 gx, u32 gy, u32 gz, u32 block, u32 lds) {
    MatchStep& s = step[n < CAP ? n++ : CAP - 1];      // (CAP is the longest plan: plan_match cannot overrun it)
    s = MatchStep();
    s.k = k; s.gx = gx; s.gy = gy; s.gz = gz; s.block = block; s.lds = lds;
    return s;
}

int match_scan1_lanes(const MatchInputs& in) {
    const ScanPlan p = plan_scan(in.scan, in.nslots, in.layouts, in.n_litems);
    return p.kind == ScanPlan::Scan1 ? p.param : 0;
}

// a11-a13: the scan of the range.  variant bits -- k_scan: 0-1 feature-loop unroll (0: 8 loads in flight, 1: 4, 2: 2), 2 plain (slot = grid.z)
// mapping instead of the XCD-aware one; k_scan4: 0-1 features per load block (0: 6, 1: 12, 2: 3), 3 no pruning (the plain exhaustive scan),
// 4 wave-level pruning only (r02's rule), 5 per-lane pruning whatever the modality count, 6 with 3 (measurement only, wrong sums): without the
// shift-undo; the bit-plane scans: 7 (measurement only, WRONG lists) no exact sums, 8 (k_scan1) the waves take their survivors' sums themselves,
// 9-11 k_scanl's timing experiments.
// k_scan4's default pruning: per-lane for two modalities (r03, config 2: 181.6 -> 172.9 us per 96-frame launch, 35 % of the lane-loads instead
// of 50 %), wave-level for one (config 3: the per-lane form measured 455 against 413 us per 128-frame launch: with 31 features per template few
// lanes die long before their wave does, and the masked loads still pull the same lines).
static void plan_scan_steps(const MatchInputs& in, MatchPlan& p) {
    const int variant = in.variant, nslots = in.nslots;
    const bool spread = in.layouts == layout_bit(Layout::SpreadAndPlanes);
    ScanPlan sp = plan_scan(in.scan, nslots, in.layouts, in.n_litems);
    // no work items for the lane count (they could not be built): slots that still have response memories take k_scan4; slots that keep only
    // the spread byte are refused -- k_scan4 would read garbage there
    if (sp.kind == ScanPlan::Scan1 && in.items1_L != sp.param) sp.kind = spread ? ScanPlan::NoBitPlaneForm : ScanPlan::Scan4;
    p.kind = sp.kind;
    if (sp.kind == ScanPlan::Mixed || sp.kind == ScanPlan::NoBitPlaneForm) return;
    p.n_items = in.n_items;
    if (sp.kind != ScanPlan::Scan4) {       // the bit-plane forms: the miss bound, the exact sums from the response memories or the spread byte
        p.delta_rcp16 = (65536u + (u32)in.miss_delta - 1u) / (u32)in.miss_delta;
        p.exact_spread = spread;
        p.no_exact = (variant & 128) ? 1 : 0;
    }
    if (sp.kind == ScanPlan::ScanL) {
        p.R = sp.param;
        p.pb = (u32)in.T * (u32)in.T * in.wh / 8u; p.planes_off = 8u * in.ori_stride;
        const u32 img = (u32)in.M * 8u * p.pb;
        p.tbl_bytes = std::max<u32>(LM_SCANL_TABLE_BYTES, (((in.wh + 127u) / 128u) * 16u + 32u + 15u) & ~15u);
        p.queue_cap = std::min<u32>((LM_SCANL_LDS_BYTES - img - p.tbl_bytes - 16u - 512u) / 4u, 1u << 16);      // (16: queue header, 512: the raw thresholds)
        p.dbg = (variant >> 9) & 7;
    } else if (sp.kind == ScanPlan::Scan1) {
        p.L1 = sp.param; p.G1 = 64 / p.L1;
        p.L1_rcp16 = (65536u + (u32)p.L1 - 1u) / (u32)p.L1;
        p.n_items = in.n_items1;
        // the queue entry's 20-bit position / 12-bit slot.  The lane moves on to the other counter set whenever a queue was handed to the launch,
        // whatever the variant does with it
        const bool handed = in.have_queue && !(in.wh >= (1u << 20) || nslots > 4096);
        p.flip_surv_set = handed;
        p.queue = handed && !(variant & 256);
        // (the two measurement variants do not run k_scan1_exact, which re-arms the other counter set for the stream's next launch: re-arm both first)
        if (p.n_items > 0 && handed && (p.no_exact || (variant & 256))) p.add(MatchKernel::SurvReset, 1, 1, 1, 0);
    }
    if (p.n_items <= 0) return;
    const int G = (p.n_items + 3) / 4;               // one wave per work item
    p.wgs_per_slot = G;
    if (sp.kind == ScanPlan::ScanL) {
        // one 1024-thread workgroup = (frame, share of the templates), the frame's planes in ALL of the CU's LDS
        p.add(MatchKernel::ScanL, (u32)(nslots * p.R), 1, 1, 1024, LM_SCANL_LDS_BYTES);
    } else if (sp.kind == ScanPlan::Scan1) {
        // a wave scans its item for a GROUP of G1 slots (XCD affinity per group when the group count allows)
        const int ngroups = (nslots + p.G1 - 1) / p.G1;
        p.add(MatchKernel::Scan1, (u32)(G * ngroups), 1, 1, 256);
        if (p.queue && !p.no_exact) p.add(MatchKernel::Scan1Exact, 1024, 1, 1, 256);
    } else if (in.nibble) {
        // k_scan4: a wave scans its item for a PAIR of slots; 1-D grid with XCD affinity per pair
        const u32 gx = (u32)(G * ((nslots + 1) / 2));
        if ((variant & 64) && (variant & 8)) { p.add(MatchKernel::Scan4NoShift, gx, 1, 1, 256); return; }
        const int fb = (variant & 3) == 1 ? 1 : (variant & 3) == 2 ? 2 : 0;
        const int prune = (variant & 8) ? 0 : ((variant & 16) || (in.M < 2 && !(variant & 32))) ? 1 : 2;
        p.add((MatchKernel)((int)MatchKernel::Scan4_6_P0 + 3 * fb + prune), gx, 1, 1, 256);
    } else {
        const bool xcd = !(variant & 4) && (nslots == 1 || nslots == 2 || nslots == 4 || (nslots % 8) == 0);
        const int u = (variant & 3) == 1 ? 1 : (variant & 3) == 2 ? 2 : 0;
        if (xcd) p.add((MatchKernel)((int)MatchKernel::Scan8X + u), (nslots % 8) == 0 ? (u32)(G * nslots) : 8u * (u32)((G + 8 / nslots - 1) / (8 / nslots)), 1, 1, 256);
        else p.add((MatchKernel)((int)MatchKernel::Scan8 + u), (u32)G, 1, (u32)nslots, 256);
    }
}

void plan_match(const MatchInputs& in, MatchPlan& p) {
    p = MatchPlan();
    plan_scan_steps(in, p);      // (a refused scan plans no scan step; the caller refuses the call)
    p.scan_end = p.n;
    const int n = in.nslots;
    if (in.L == 1) {        // candidates become matches unrefined
        p.add(MatchKernel::EmitUnrefined, 64, 1, (u32)n, 256);
    } else {
        // 8+ slots: balance the slots over the XCDs by their candidate counts (one plan per lane)
        p.plan_cap = n / 8 + 8;      // pieces per XCD list: its share of the slots + room for the pieces of the heavy ones
        p.refine_plan = (n % 8) == 0 && n <= 1016 && p.plan_cap <= in.plan_stride_cap && in.have_plan;
        if (p.refine_plan) p.add(MatchKernel::RefinePlan, 1, 1, 1, 1024);
        // persistent waves stride over the slot's candidate list; with the XCD-affine mapping one slot runs on one XCD (32 CUs x 32 waves), so 256
        // blocks = 1024 waves per slot fill it.  With a plan the 256 workgroups of XCD x (8 per CU) are one queue over the candidates of the slots
        // on its list
        for (int l = in.L - 2; l >= 0; --l) {
            const bool w4 = (in.level_W[l] & 3) == 0;     // the patch rows' pitch: scalar alignment arithmetic in rf_patch
            const MatchKernel k = l == 0 ? (w4 ? MatchKernel::RefineLastW4 : MatchKernel::RefineLast) : (w4 ? MatchKernel::RefineW4 : MatchKernel::Refine);
            p.add(k, p.refine_plan ? (u32)(8 * p.blocks_per_slot) : (u32)(p.blocks_per_slot * n), 1, 1, 256).level = (unsigned char)l;
        }
    }
    p.refine_end = p.n;
    // split form (four chunk workgroups per frame + a merge launch) when this detector's recent lists were long enough to need it: the lists are
    // identical either way, so the choice may follow what the last collected frames looked like
    p.split = in.sort_split_mode == 1 || (in.sort_split_mode == 2 && in.sort_long_score > 0);
    const u32 lds = (u32)LM_SORT_CAP * 16u;
    p.add(MatchKernel::SortUnique, 1, p.split ? LM_SORT_CAP / LM_SORT_CHUNK : 1, (u32)n, 1024, lds);
    if (p.split) p.add(MatchKernel::MergeUnique, 1, 1, (u32)n, 1024, lds);
}

// ================================================================================================
// The ICP batch planner (lm_host.h).
// ================================================================================================
namespace {
inline size_t icp_align(size_t v) { return (v + 255) / 256 * 256; }
inline int icp_tiles(long long n) { return (int)((n + LM_ICP_TILE - 1) / LM_ICP_TILE); }
inline int cv_round(double x) { return (int)std::nearbyint(x); }   // half to even under the default rounding mode, like cvRound

// Lays out a chunk of the queries in c.q (their sizes set): the chunk's tables first, then every query's regions.
void icp_layout(IcpChunkPlan& c, int levels) {
    const size_t nq = c.q.size();
    size_t o = 0;
    const auto take = [&o](size_t bytes) { const size_t at = o; o = icp_align(o + std::max<size_t>(bytes, 1)); return at; };
    c.np = 0; c.g_px = 0; c.g_normals = 0; c.nlevels = levels;
    for (const IcpQueryPlan& e : c.q) c.np += e.np;
    c.zsum = take(nq * 8);
    c.counts = take(nq * 2 * sizeof(u32));
    c.scene_recs = take(nq * sizeof(LmIcpSceneRec));
    c.reg_recs = take(nq * sizeof(LmIcpRegRec));
    c.levels = take(nq * (size_t)levels * sizeof(LmIcpLevel));
    c.st = take((size_t)c.np * sizeof(LmIcpPose));
    c.out = take((size_t)c.np * 16 * sizeof(double));
    for (IcpQueryPlan& e : c.q) {
        const size_t np = (size_t)e.np, nm = (size_t)e.nm, ns = (size_t)e.ns_cap;
        e.z = take((size_t)e.npx * 4);
        e.blockcnt = take((size_t)e.nb * 4);
        e.blockoff = take((size_t)e.nb * 4);
        e.cloud = take((ns + 1) * 6 * sizeof(float));
        e.src0 = take(np * nm * 6 * 8);
        e.srcL = take(np * nm * 6 * 8);
        e.part = take(np * (size_t)e.nch_cap * nm * sizeof(LmIcpNN));
        e.nd = take(np * nm * 4);
        e.nidx = take(np * nm * 4);
        e.keys = take(np * ns * 8);
        e.acc = take(np * (size_t)e.nblk_cap * LM_ICP_ACC * 8);
        c.g_px = std::max(c.g_px, (u32)e.nb);
        c.g_normals = std::max(c.g_normals, (u32)icp_tiles((long long)ns + 1));
    }
    c.bytes = o;
}
}  // namespace

std::vector<IcpRegion> IcpChunkPlan::regions() const {
    const size_t nq = q.size();
    std::vector<IcpRegion> r;
    r.push_back({"zsum", -1, zsum, nq * 8});
    r.push_back({"counts", -1, counts, nq * 2 * sizeof(u32)});
    r.push_back({"scene_recs", -1, scene_recs, nq * sizeof(LmIcpSceneRec)});
    r.push_back({"reg_recs", -1, reg_recs, nq * sizeof(LmIcpRegRec)});
    r.push_back({"levels", -1, levels, nq * (size_t)nlevels * sizeof(LmIcpLevel)});
    r.push_back({"st", -1, st, (size_t)np * sizeof(LmIcpPose)});
    r.push_back({"out", -1, out, (size_t)np * 16 * sizeof(double)});
    for (const IcpQueryPlan& e : q) {
        const size_t n = (size_t)e.np, nm = (size_t)e.nm, ns = (size_t)e.ns_cap;
        r.push_back({"z", e.query, e.z, (size_t)e.npx * 4});
        r.push_back({"blockcnt", e.query, e.blockcnt, (size_t)e.nb * 4});
        r.push_back({"blockoff", e.query, e.blockoff, (size_t)e.nb * 4});
        r.push_back({"cloud", e.query, e.cloud, (ns + 1) * 6 * sizeof(float)});
        r.push_back({"src0", e.query, e.src0, n * nm * 6 * 8});
        r.push_back({"srcL", e.query, e.srcL, n * nm * 6 * 8});
        r.push_back({"part", e.query, e.part, n * (size_t)e.nch_cap * nm * sizeof(LmIcpNN)});
        r.push_back({"nd", e.query, e.nd, n * nm * 4});
        r.push_back({"nidx", e.query, e.nidx, n * nm * 4});
        r.push_back({"keys", e.query, e.keys, n * ns * 8});
        r.push_back({"acc", e.query, e.acc, n * (size_t)e.nblk_cap * LM_ICP_ACC * 8});
    }
    return r;
}

void plan_icp_batch(const std::vector<IcpQueryIn>& q, int step, int levels, size_t budget, IcpBatchPlan& p) {
    p = IcpBatchPlan();
    IcpChunkPlan cur;
    for (size_t k = 0; k < q.size(); ++k) {
        const IcpQueryIn& in = q[k];
        if (in.np <= 0) continue;
        IcpQueryPlan e;
        e.query = (int)k; e.npx = in.npx; e.nb = icp_tiles(in.npx); e.nm = in.nm; e.np = in.np;
        e.ns_cap = std::max(in.npx / step, 1);
        e.nch_cap = lm_icp_nn_chunks(e.ns_cap);
        e.nblk_cap = std::max(1, icp_tiles(e.ns_cap));
        bool fresh = cur.q.empty();
        for (const IcpQueryPlan& o : cur.q) {       // overlapping pose ranges keep their sequential meaning: the later query reads the earlier one's result
            const IcpQueryIn& a = q[(size_t)o.query];
            if (in.first_pose < a.first_pose + a.np && a.first_pose < in.first_pose + in.np) fresh = true;
        }
        if (!fresh) {
            IcpChunkPlan with = cur;
            with.q.push_back(e);
            icp_layout(with, levels);
            if (with.bytes <= budget) { cur = with; continue; }
        }
        if (!cur.q.empty()) p.chunks.push_back(cur);
        cur = IcpChunkPlan();
        cur.q.push_back(e);
        icp_layout(cur, levels);
    }
    if (!cur.q.empty()) p.chunks.push_back(cur);
}

// The level schedule of registerModelToScene for a model of n rows and a scene of ns rows, coarsest level first.  fval_perc starts at
// 0, so a level iterates only while TolP = tolerance (level + 1)^2 <= 1 (the loop test !(fval_perc < 1 + TolP && fval_perc > 1 - TolP));
// a level whose clouds sample fewer than 6 rows cannot pair 6 points and stops at once.
std::vector<LmIcpLevel> icp_schedule(int n, int ns, int iterations, int levels, double tolerance) {
    std::vector<LmIcpLevel> out;
    for (int level = levels - 1; level >= 0; --level) {
        LmIcpLevel L{};
        L.level = level;
        const int num = std::max(cv_round((double)n / std::ldexp(1.0, level)), 1);
        L.s = std::max(cv_round((double)n / (double)num), 1);
        L.nL = n / L.s;
        L.ndL = ns / L.s;
        L.tolp = tolerance * (double)(level + 1) * (double)(level + 1);
        L.max_it = cv_round((double)iterations / (double)(level + 1));
        L.rounds = (L.tolp <= 1.0 && L.nL >= 6 && L.ndL >= 6) ? L.max_it : 0;
        out.push_back(L);
    }
    return out;
}

void plan_icp_levels(const IcpChunkPlan& c, const std::vector<int>& scene_rows, int iterations, int levels, double tolerance, IcpLevelsPlan& p) {
    p = IcpLevelsPlan();
    p.nlevels = levels;
    p.pose0.assign(c.q.size(), -1);
    p.lev.assign(c.q.size() * (size_t)levels, LmIcpLevel{});
    p.level.assign((size_t)levels, IcpLevelLaunch());
    for (size_t k = 0; k < c.q.size(); ++k) {
        if (scene_rows[k] < 0) continue;
        p.pose0[k] = p.np;
        p.np += c.q[k].np;
        const std::vector<LmIcpLevel> s = icp_schedule(c.q[k].nm, scene_rows[k], iterations, levels, tolerance);
        for (int l = 0; l < levels; ++l) {
            const LmIcpLevel& L = s[(size_t)l];
            p.lev[k * (size_t)levels + (size_t)l] = L;
            if (L.rounds == 0) continue;
            IcpLevelLaunch& g = p.level[(size_t)l];
            g.rounds = std::max(g.rounds, L.rounds);
            g.g_src = std::max(g.g_src, (u32)icp_tiles(L.nL));
            g.g_chunks = std::max(g.g_chunks, (u32)lm_icp_nn_chunks(L.ndL));
            g.g_dst = std::max(g.g_dst, (u32)std::max(1, icp_tiles(L.ndL)));
        }
    }
}

// ================================================================================================
// The pre-processing planner (lm_host.h): a call's description -> the ordered launches of a3-a10.
// ================================================================================================
namespace {
struct PreTuning {     // process-wide; relaxed: a snapshot needs no order between the knobs, only whole values
    std::atomic<int> cblur_variant{0}, cgrad_variant{0}, pyrdown_variant{0}, dmedian_variant{0};
    std::atomic<int> blur_pyr{1}, blur_pyr_interleave{2}, blur_strip{0}, cgrad_levels{1};
} g_pre_tuning;
}  // namespace

PreKnobs pre_knobs() {
    const auto get = [](const std::atomic<int>& a) { return a.load(std::memory_order_relaxed); };
    PreKnobs k;
    k.cblur_variant = get(g_pre_tuning.cblur_variant); k.cgrad_variant = get(g_pre_tuning.cgrad_variant);
    k.pyrdown_variant = get(g_pre_tuning.pyrdown_variant); k.dmedian_variant = get(g_pre_tuning.dmedian_variant);
    k.blur_pyr = get(g_pre_tuning.blur_pyr); k.blur_pyr_interleave = get(g_pre_tuning.blur_pyr_interleave);
    k.blur_strip = get(g_pre_tuning.blur_strip); k.cgrad_levels = get(g_pre_tuning.cgrad_levels);
    return k;
}

bool set_pre_knob(int key, int v) {
    const auto set = [](std::atomic<int>& a, int x) { a.store(x, std::memory_order_relaxed); return true; };
    switch (key) {
        case LM_TUNE_CBLUR_VARIANT: return v >= 0 && v <= 4 && v != 2 && set(g_pre_tuning.cblur_variant, v);      // (2 was r02's k_cblur_sw, deleted in r05)
        case LM_TUNE_CGRAD_VARIANT: return v >= 0 && v <= 3 && set(g_pre_tuning.cgrad_variant, v);
        case LM_TUNE_PYRDOWN_VARIANT: return v >= 0 && v <= 2 && set(g_pre_tuning.pyrdown_variant, v);
        case LM_TUNE_DMEDIAN_VARIANT: return v >= 0 && v <= 2 && set(g_pre_tuning.dmedian_variant, v);
        case LM_TUNE_BLUR_PYR:      // 0: two launches, 1: one launch, 2: ... its tiles always dealt evenly, 3: ... for frames of more than 2 MB
            return v >= 0 && v <= 3 && set(g_pre_tuning.blur_pyr, v != 0) && set(g_pre_tuning.blur_pyr_interleave, v == 2 ? 1 : v == 3 ? 2 : 0);
        case LM_TUNE_BLUR_STRIP: return (v == 0 || v == 16 || v == 32 || v == 64) && set(g_pre_tuning.blur_strip, v);
        case LM_TUNE_CGRAD_LEVELS: return v >= 0 && v <= 1 && set(g_pre_tuning.cgrad_levels, v);
        default: return false;
    }
}

const char* pre_kernel_name(PreKernel k) {
    static const char* const names[(int)PreKernel::Count] = {
        "k_pyrdown", "k_pyrdown8", "k_pyrdown16", "k_nn_half",
        "k_blur_pyr<16>", "k_blur_pyr<32>", "k_blur_pyr<64>", "k_blur_mx_pyr",
        "k_cblur", "k_cblur_sh<16>", "k_cblur_sh<32>", "k_cblur_mx",
        "k_corient", "k_cvote", "k_cgrad<8>", "k_cgrad<16>", "k_cgrad<32>", "k_color_quantize",
        "k_cgrad_levels<32,16>", "k_cgrad_levels<32,8>", "k_cgrad_levels<16,16>", "k_cgrad_levels<16,8>", "k_cgrad_levels<8,8>",
        "k_dnormal", "k_dmedian<4>", "k_dmedian<16>", "k_depth_quantize",
        "mask_rules", "match_masks",
        "k_lm_spread2", "k_lm_spread5", "k_lm_fast<2,128>", "k_lm_fast<4,64>", "k_lm_fast<5,128>", "k_lm_fast<8,40>", "k_lm_fast<8,80>", "k_linear_memories",
        "k_phase<1,5>", "k_phase<2,5>", "k_phase<3,5>", "k_phase<4,5>", "k_phase<4,2>",
        "k_bsplit<0,16>", "k_bsplit<1,16>", "k_bsplit<1,32>", "k_bsplit<2,16>",
        "k_bphase<1,5,16,16>", "k_bphase<2,5,16,16>", "k_bphase<3,5,16,16>", "k_bphase<1,5,32,32>", "k_bphase<2,5,32,32>", "k_bphase<3,5,32,32>",
        "k_bphase<1,2,16,16>", "k_bphase<2,2,16,16>", "k_bphase<3,2,16,16>", "k_bphase<1,2,32,32>", "k_bphase<2,2,32,32>", "k_bphase<3,2,32,32>",
    };
    return k < PreKernel::Count ? names[(int)k] : "?";
}

PreStep& PrePlan::add(PreKernel k, int level, int modality) {
    assert(n < CAP);      // (CAP is the longest plan there is: see lm_host.h)
    PreStep& s = step[n < CAP ? n++ : CAP - 1];
    s = PreStep();
    s.k = k; s.level = (unsigned char)level; s.modality = (unsigned char)modality;
    return s;
}

namespace {

typedef PreKernel K;

// Kernel selection is by WORK, not by frame count (r04): the few-frame kernels (many short waves, finish sooner) and the batch kernels
// (row-walking, fewer instructions per pixel) were tuned on 640 x 480 frames, where the break-even is 16 frames.  A call's frames count
// `weight` times: eight 1280 x 960 frames (config 5) carry the pixels of 32 VGA frames and take the batch kernels.
bool batch(const PreInputs& in) { return in.n * in.weight >= 16; }

// a launch of g blocks per slot over the call's slots
PreStep& add_slots(PrePlan& p, K k, int l, int m, int g, const PreInputs& in) {
    PreStep& s = p.add(k, l, m);
    s.gx = (u32)(g * in.n); s.pg.g[0] = g;
    return s;
}
// a launch on a 2-D grid of tiles, one plane per slot
void add_tiles(PrePlan& p, K k, int l, int m, int gx, int gy, const PreInputs& in) {
    PreStep& s = p.add(k, l, m);
    s.gx = (u32)gx; s.gy = (u32)gy; s.gz = (u32)in.n;
}
// a fused launch: up to four parts, each on its own range of the block index
void add_fused(PrePlan& p, K k, const LmPhaseGrid& pg) {
    PreStep& s = p.add(k, 0, 0);
    s.pg = pg; s.gx = pg.nb[0] + pg.nb[1] + pg.nb[2] + pg.nb[3];
}

// ---- the shapes the streaming kernels take
// the 4-pass colour kernels (blur | orientation | vote, or blur | fused gradient): 16-byte lanes on every image
bool color_streams(const PreInputs& in, int l) {
    const PreLevel& v = in.lv[l];
    return (v.w % 16) == 0 && v.a_bgr == 0 && v.a_cs == 0 && v.a_quant[0] == 0 && in.a_stride == 0;
}
// the blur alone does not touch the quantised image
bool blur_streams(const PreInputs& in, int l) {
    const PreLevel& v = in.lv[l];
    return (v.w % 16) == 0 && v.a_bgr == 0 && v.a_cs == 0 && in.a_stride == 0;
}
// k_pyrdown8 / k_pyrdown16: 16-byte loads, 8-byte stores
bool pyrdown_streams(const PreInputs& in, int l) {
    return (in.lv[l - 1].w % 16) == 0 && in.lv[l - 1].a_bgr == 0 && (in.lv[l].a_bgr & 7) == 0 && in.a_stride == 0;
}
bool pyrdown16_shape(const PreInputs& in, int l) { return pyrdown_streams(in, l) && (in.lv[l - 1].h % 2) == 0 && in.lv[l - 1].h >= 4; }
// k_dnormal + k_dmedian (counting median: one-hot labels)
bool depth_streams(const PreInputs& in) {
    return in.lut_onehot && (in.lv[0].w % 8) == 0 && in.a_depth == 0 && (in.a_ds & 7) == 0 && (in.lv[0].a_quant[1] & 7) == 0 && in.a_stride == 0;
}
// k_lm_spread5: eight positions per lane
bool spread5_shape(const PreInputs& in, int l, int m) {
    const PreLevel& v = in.lv[l];
    const int W = v.w / 5;
    return (W % 8) == 0 && (v.h % 5) == 0 && (v.a_lm[m] & 7) == 0 && (in.a_stride & 7) == 0 && (((size_t)W * (v.h / 5)) % 8) == 0;
}
// the second level is exactly half the first (the fused routes compute it as w / 2 x h / 2)
bool half_size(const PreInputs& in) { return in.lv[1].w * 2 == in.lv[0].w && in.lv[1].h * 2 == in.lv[0].h; }

// ---- the blur of one level launched alone
enum class Blur { OneShot, Shared, Matrix };
// the matrix cores by default for batches of frames of up to 2 MB: alone on the chip no faster than k_cblur_sh, beside the other lanes
// config 2 +1.5 .. 2 % (the vector ALU is what the pipeline is short of), config 3 -0.8 % (HBM-bound launch)
bool mx_auto(const PreInputs& in, int w, int h) { return in.knobs.cblur_variant == 0 && batch(in) && (long)w * h * 3 <= 2000000L && ((w * 3) % 32) == 0; }
bool mx_wanted(const PreInputs& in, int w, int h) { return in.knobs.cblur_variant == 4 || mx_auto(in, w, h); }
Blur pick_blur(const PreInputs& in, int l) {
    const int w = in.lv[l].w, h = in.lv[l].h, v = in.knobs.cblur_variant;
    if (mx_wanted(in, w, h) && ((w * 3) % 32) == 0 && h >= 1) return Blur::Matrix;
    // few frames: the one-shot kernel's many short waves finish sooner (a single frame is 57 sliding-window waves of eight dependent
    // steps: 166 instead of 150 us per resident single-frame match); batches: the sliding window
    return v == 1 || (v == 0 && !batch(in)) ? Blur::OneShot : Blur::Shared;
}
void add_blur(const PreInputs& in, int l, Blur b, PrePlan& p) {
    const int w = in.lv[l].w, h = in.lv[l].h;
    if (b == Blur::Matrix) {
        const MxGrid g = cblur_mx_grid(w, h, in.knobs.blur_strip);
        PreStep& s = add_slots(p, K::CblurMx, l, 0, g.gx * g.gy, in);
        s.param = g.rows; s.pg.g[0] = g.gx; s.pg.g[1] = g.gy;
    } else if (b == Blur::OneShot) {
        add_slots(p, K::Cblur, l, 0, cblur_blocks(w, h), in);
    } else {
        const int strip = cblur_sh_strip(h);
        add_slots(p, strip == 32 ? K::CblurSh32 : K::CblurSh16, l, 0, cblur_sh_blocks(w, h, strip), in);
    }
}
K cgrad_kernel(int strip) { return strip == 32 ? K::Cgrad32 : strip == 16 ? K::Cgrad16 : K::Cgrad8; }

// Batches: the level-0 blur AND cv::pyrDown level 0 -> 1 in one slot-interleaved launch, so that the raw image comes from HBM once.
// false: nothing planned (exactly the shapes the streaming colour kernels and k_pyrdown16 take, batches only).
bool plan_blur_pyrdown(const PreInputs& in, PrePlan& p) {
    const PreKnobs& kn = in.knobs;
    const int w = in.lv[0].w, h = in.lv[0].h;
    if (!kn.blur_pyr || !batch(in) || kn.cblur_variant == 1 || kn.cblur_variant == 2 || kn.pyrdown_variant == 1) return false;
    if (!color_streams(in, 0) || !pyrdown16_shape(in, 1)) return false;
    const int g_pyr = pyrdown16_blocks(w, h);
    if (mx_wanted(in, w, h)) {
        if (((w * 3) % 32) != 0) return false;
        const MxGrid g = cblur_mx_grid(w, h, kn.blur_strip);
        PreStep& s = add_slots(p, K::BlurMxPyr, 0, 0, g.gx * g.gy + g_pyr, in);
        s.param = g.rows; s.pg.g[0] = g.gx; s.pg.g[1] = g.gy; s.pg.g[2] = g_pyr;
        return true;
    }
    // rows per blur strip: 16, or 32 for tall images.  A strip of S rows reads and sums S + 6 (16: 1.375 x the image, 32: 1.19 x, 64:
    // 1.09 x) but taller strips measured no faster (r03: config 2 163.2 / 162.8 / 160.8 K detections/s at 16 / 32 / 64): fewer, longer waves
    int strip = CBS_STRIP;
    if (kn.blur_strip == 64) strip = 64;
    // DIFFERS from cblur_sh_strip: k_blur_pyr's own rule -- 32-row strips only when they still give the chip three rounds of workgroups
    // (eight 1280 x 960 frames, config 5, are 312 workgroups of 32-row strips on 512 slots)
    else if (kn.blur_strip == 32 || (kn.blur_strip == 0 && h > 640 && (long)(cblur_sh_blocks(w, h, 32) + g_pyr) * in.n >= 768)) strip = 32;
    const int g_blur = cblur_sh_blocks(w, h, strip);
    PreStep& s = add_slots(p, strip == 64 ? K::BlurPyr64 : strip == 32 ? K::BlurPyr32 : K::BlurPyr16, 0, 0, g_blur + g_pyr, in);
    s.pg.g[0] = g_blur; s.pg.g[1] = g_pyr;
    // tiles dealt evenly by rows: 1280 x 960 reads 8.64 -> 7.54 MB per frame (config 3 +0.8 %); 640 x 480 gets 4 us LONGER per launch
    s.param = kn.blur_pyr_interleave == 1 || (kn.blur_pyr_interleave == 2 && (long)w * h * 3 > 2000000L);
    return true;
}

// r06: a batch's level-0 and level-1 gradients in one grid (level 1's few waves fill the idle SIMDs of level 0's last round)
bool cgrad_levels_shape(const PreInputs& in) {
    const int v = in.knobs.cgrad_variant;
    return in.knobs.cgrad_levels != 0 && (v == 0 || v == 2 || v == 3) && batch(in) && (in.lv[0].w % 32) == 0 && (in.lv[0].h % 2) == 0 &&
           in.lv[0].a_cs == 0 && in.lv[1].a_cs == 0 && in.lv[0].a_quant[0] == 0 && in.lv[1].a_quant[0] == 0 && in.a_stride == 0 && (in.lv[1].w % 16) == 0;
}
void plan_cgrad_levels(const PreInputs& in, PrePlan& p) {
    const PreLevel &v0 = in.lv[0], &v1 = in.lv[1];
    // level 0's strip as for a launch of its own; level 1: 16 rows when it alone fills the chip, 8 otherwise
    const int s0 = cgrad_strip(v0.w, v0.h, in.n, in.knobs.cgrad_variant == 3), s1 = cgrad_strip_upper(v1.w, v1.h, in.n);
    const int g0 = cgrad_blocks(v0.w, v0.h, s0), g1 = cgrad_blocks(v1.w, v1.h, s1);
    const K k = s0 == 32 ? (s1 == 16 ? K::CgradLevels32_16 : K::CgradLevels32_8) : s0 == CG_STRIP ? (s1 == 16 ? K::CgradLevels16_16 : K::CgradLevels16_8) : K::CgradLevels8_8;
    PreStep& s = add_slots(p, k, 0, 0, g0 + g1, in);
    s.pg.g[0] = g0; s.pg.g[1] = g1;
}

void plan_mode_lm_fast(PrePlan& p, K k, int seg, int l, int m, bool src_shift, const PreInputs& in) {
    const PreLevel& v = in.lv[l];
    const int nseg = lm_fast_segs(v.w / v.T, seg);
    PreStep& s = add_slots(p, k, l, m, nseg * (v.h / v.T), in);
    s.pg.g[0] = nseg; s.src_shift = src_shift;
}

// ---- a3-a10 of FEW frames as five launches instead of fourteen: the kernels of one dependency level side by side
//   1  blur(level 0)            | depth normals          | pyrDown(level 0 -> 1)
//   2  median of the normals    | blur(level 1)          | orientation(level 0)
//   3  vote(level 0)            | orientation(level 1)   | depth linear memories of levels 0 and 1
//   4  vote(level 1)            | colour linear memories of level 0
//   5  colour linear memories of level 1
// (the default two-level RGB-D / colour pyramid with T = {5, 8}, or {2, 8} without depth, only)
bool phases_shape(const PreInputs& in) {
    const PreLevel &v0 = in.lv[0], &v1 = in.lv[1];
    const bool dep = in.M == 2;
    if (in.L != 2 || in.M > 2 || !half_size(in) || in.n < 1) return false;
    if ((v0.T != 5 && !(v0.T == 2 && !dep)) || v1.T != 8 || v0.mode != 1 || v1.mode != 2) return false;
    if ((v0.w % 32) != 0 || (v0.h % 2) != 0) return false;
    if (!color_streams(in, 0) || !color_streams(in, 1) || !pyrdown_streams(in, 1) || (dep && !depth_streams(in))) return false;
    if (!nibble_supported(v1.w, 8) || (v1.w / 8) % 4 != 0) return false;                                   // k_lm_fast<8, 40, ., 2>
    if (v0.T == 5 && (v0.w / 5) % 4 != 0) return false;                                                      // k_lm_fast<5, 128, ., 1>
    if (v0.T == 2 && (v0.a_lm[0] != 0 || (((size_t)(v0.w / 2) * (v0.h / 2)) % 16) != 0)) return false;     // k_lm_spread2
    return true;
}
void plan_phases(const PreInputs& in, PrePlan& p) {
    const int w = in.lv[0].w, h = in.lv[0].h, w1 = w / 2, h1 = h / 2, n = in.n, T0 = in.lv[0].T;
    const bool dep = in.M == 2;
    const int g_blur0 = cblur_blocks(w, h), g_blur1 = cblur_blocks(w1, h1);
    const int g_ori0 = corient_blocks(w, h), g_ori1 = corient_blocks(w1, h1);
    const int g_vote0 = cvote_blocks(w, h), g_vote1 = cvote_blocks(w1, h1);
    const int g_pyr = pyrdown8_blocks(w, h), g_nrm = dnormal_blocks(w, h), g_med = dmedian_blocks(w, h, DM_ROWS);
    // linear memories: segments per band (k_lm_fast); for T0 = 2 the streaming kernel's blocks per slot instead
    const int seg0 = T0 == 5 ? lm_fast_segs(w / 5, 128) : lm_spread2_blocks(w, h), seg1 = lm_fast_segs(w1 / 8, 40);
    const u32 b_lm0 = T0 == 5 ? (u32)(seg0 * (h / 5) * n) : (u32)(seg0 * n), b_lm1 = (u32)(seg1 * (h1 / 8) * n);
    add_fused(p, K::Phase1, {{(u32)(g_blur0 * n), dep ? (u32)(g_nrm * n) : 0u, (u32)(g_pyr * n), 0u}, {g_blur0, g_nrm, g_pyr, 0}});
    add_fused(p, K::Phase2, {{dep ? (u32)(g_med * n) : 0u, (u32)(g_blur1 * n), (u32)(g_ori0 * n), 0u}, {g_med, g_blur1, g_ori0, 0}});
    add_fused(p, K::Phase3, {{(u32)(g_vote0 * n), (u32)(g_ori1 * n), dep ? b_lm0 : 0u, dep ? b_lm1 : 0u}, {g_vote0, g_ori1, seg0, seg1}});
    add_fused(p, T0 == 5 ? K::Phase4_T5 : K::Phase4_T2, {{(u32)(g_vote1 * n), b_lm0, 0u, 0u}, {g_vote1, seg0, 0, 0}});
    // DIFFERS from plan_linear_memories: the few-frame route never takes k_lm_fast<8, 80>
    plan_mode_lm_fast(p, K::LmFast8_40, 40, 1, 0, false, in);
}

// ---- a3-a10 of a BATCH on a lone lane: the batch kernels of one dependency level share one grid (k_bphase, colour only), or, for
// RGB-D, only kernels of one register class do (k_bsplit) between plain launches
bool batch_phases_shape(const PreInputs& in) {
    if (!phases_shape(in) || !batch(in)) return false;
    if (in.lv[0].T == 5) return (in.lv[0].w % 5) == 0 && spread5_shape(in, 0, 0) && (in.M < 2 || spread5_shape(in, 0, 1));
    return in.M < 2;     // T0 == 2 is the colour-only pyramid
}
void plan_batch_phases(const PreInputs& in, PrePlan& p) {
    const PreLevel &v0 = in.lv[0], &v1 = in.lv[1];
    const int w = v0.w, h = v0.h, w1 = w / 2, h1 = h / 2, n = in.n, T0 = v0.T;
    const bool tall = h > 640;
    const int sb = cblur_sh_strip(h);
    // DIFFERS from cgrad_strip: the fused launches take 32-row gradient strips for every tall image, whatever the wave count
    const int sg = tall ? 32 : 16;
    const int g_nrm = dnormal_blocks(w, h), g_blur0 = cblur_sh_blocks(w, h, sb), g_pyr = pyrdown16_blocks(w, h);
    const int g_grad0 = cgrad_blocks(w, h, sg), g_med = dmedian_blocks(w, h, DM_ROWS_BATCH), g_blur1 = cblur_sh_blocks(w1, h1, 16);
    const int g_grad1 = cgrad_blocks(w1, h1, 16);
    const int g_sp = T0 == 5 ? lm_spread5_blocks(w, h) : lm_spread2_blocks(w, h);
    const int seg1 = lm_fast_segs(w1 / 8, 40);
    const u32 b_lm1 = (u32)(seg1 * (h1 / 8) * n);
    if (in.M == 2) {
        if (plan_blur_pyrdown(in, p)) {
            // blur(0) and pyrDown share the slot-interleaved launch (one read of the raw image); the normals go alone
            add_slots(p, K::Dnormal, 0, 1, g_nrm, in);
        } else {
            add_fused(p, K::Bsplit0, {{(u32)(g_nrm * n), (u32)(g_pyr * n), 0u, 0u}, {g_nrm, g_pyr, 0, 0}});
            // DIFFERS from pick_blur: this fallback never takes the matrix-core blur
            add_slots(p, tall ? K::CblurSh32 : K::CblurSh16, 0, 0, g_blur0, in);
        }
        add_fused(p, tall ? K::Bsplit1_32 : K::Bsplit1_16, {{(u32)(g_grad0 * n), (u32)(g_blur1 * n), 0u, 0u}, {g_grad0, g_blur1, 0, 0}});
        add_slots(p, K::Dmedian16, 0, 1, g_med, in);
        // level 1 alone: 8-row strips when 16-row ones would leave SIMDs without a wave
        const int s1 = cgrad_strip_upper(w1, h1, n);
        add_slots(p, cgrad_kernel(s1), 1, 0, cgrad_blocks(w1, h1, s1), in);
        add_fused(p, K::Bsplit2, {{(u32)(g_sp * n), (u32)(g_sp * n), b_lm1, 0u}, {g_sp, g_sp, seg1, 0}});
    } else {
        const bool bp = plan_blur_pyrdown(in, p);     // launch 1, slot-interleaved (one read of the raw image)
        static const K table[2][2][3] = {{{K::Bphase1_T5_16, K::Bphase2_T5_16, K::Bphase3_T5_16}, {K::Bphase1_T5_32, K::Bphase2_T5_32, K::Bphase3_T5_32}},
                                         {{K::Bphase1_T2_16, K::Bphase2_T2_16, K::Bphase3_T2_16}, {K::Bphase1_T2_32, K::Bphase2_T2_32, K::Bphase3_T2_32}}};
        const auto kern = [&](int ph) { return table[T0 == 5 ? 0 : 1][tall ? 1 : 0][ph - 1]; };
        if (!bp) add_fused(p, kern(1), {{0u, (u32)(g_blur0 * n), (u32)(g_pyr * n), 0u}, {g_nrm, g_blur0, g_pyr, 0}});
        add_fused(p, kern(2), {{(u32)(g_grad0 * n), 0u, (u32)(g_blur1 * n), 0u}, {g_grad0, g_med, g_blur1, 0}});
        add_fused(p, kern(3), {{(u32)(g_grad1 * n), (u32)(g_sp * n), 0u, 0u}, {g_grad1, g_sp, g_sp, seg1}});
    }
    const bool wide = lm_fast8_wide(w1 / 8, h1, v1.mode, v1.a_lm[0], in.a_stride, in.ori_stride, in.planes);
    plan_mode_lm_fast(p, wide ? K::LmFast8_80 : K::LmFast8_40, wide ? 80 : 40, 1, 0, false, in);
}

}  // namespace

void plan_pyrdown(const PreInputs& in, int l, PrePlan& p) {
    const int sw = in.lv[l - 1].w, sh = in.lv[l - 1].h, v = in.knobs.pyrdown_variant;
    if (v != 1 && (v == 2 || batch(in)) && pyrdown16_shape(in, l)) add_slots(p, K::Pyrdown16, l, 0, pyrdown16_blocks(sw, sh), in);
    else if (pyrdown_streams(in, l)) add_slots(p, K::Pyrdown8, l, 0, pyrdown8_blocks(sw, sh), in);
    else add_tiles(p, K::Pyrdown, l, 0, pre_ceil(sw / 2, 64), pre_ceil(sh / 2, 4), in);
}

void plan_nn_half(const PreInputs& in, int l, PrePlan& p) { add_tiles(p, K::NnHalf, l, 1, pre_ceil(in.lv[l].w, 64), pre_ceil(in.lv[l].h, 4), in); }

void plan_color_quantize(const PreInputs& in, int l, bool blurred, PrePlan& p) {
    const int w = in.lv[l].w, h = in.lv[l].h, v = in.knobs.cgrad_variant;
    if (!color_streams(in, l)) { add_tiles(p, K::ColorQuantize, l, 0, pre_ceil(w, CT_W), pre_ceil(h, CT_H), in); return; }
    if (!blurred) add_blur(in, l, pick_blur(in, l), p);      // (blurred: plan_blur_pyrdown left the blurred image in the level's scratch)
    // orientation + vote: fused for batches (k_cgrad), two kernels for few frames (many short waves) and whenever the caller wants the
    // magnitude image
    if (!in.want_mag && (v >= 2 || (v == 0 && batch(in)))) {
        const int strip = cgrad_strip(w, h, in.n, v == 3);
        add_slots(p, cgrad_kernel(strip), l, 0, cgrad_blocks(w, h, strip), in);
        return;
    }
    add_slots(p, K::Corient, l, 0, corient_blocks(w, h), in);
    add_slots(p, K::Cvote, l, 0, cvote_blocks(w, h), in);
}

void plan_depth_quantize(const PreInputs& in, PrePlan& p) {
    const int w = in.lv[0].w, h = in.lv[0].h, v = in.knobs.dmedian_variant;
    if (!depth_streams(in)) { add_tiles(p, K::DepthQuantize, 0, 1, pre_ceil(w, DT_W), pre_ceil(h, DT_H), in); return; }
    const bool dm_batch = v == 2 || (v == 0 && batch(in));
    add_slots(p, K::Dnormal, 0, 1, dnormal_blocks(w, h), in);
    add_slots(p, dm_batch ? K::Dmedian16 : K::Dmedian4, 0, 1, dmedian_blocks(w, h, dm_batch ? DM_ROWS_BATCH : DM_ROWS), in);
}

void plan_linear_memories(const PreInputs& in, int l, int m, u32 planes, PrePlan& p) {
    const PreLevel& v = in.lv[l];
    // level l > 0 of the depth modality reads the quantised image of level l - 1 at (2y, 2x)
    const bool sh = m != 0 && l != 0;
    const int w = v.w, h = v.h, T = v.T, W = w / T, mode = v.mode;
    const int qpitch = sh ? in.lv[l - 1].w : w;
    const u32 a_q = sh ? in.lv[l - 1].a_quant[1] : v.a_quant[m], a_lm = v.a_lm[m];
    if ((w % 4) == 0 && (W % 4) == 0 && (qpitch % 4) == 0 && (a_q & 3) == 0 && (in.a_stride & 3) == 0) {
        switch (T) {
            case 2:
                if (mode == 1 && !sh && (w % 32) == 0 && (h % 2) == 0 && (qpitch % 16) == 0 && a_q == 0 && a_lm == 0 && in.a_stride == 0 && (((size_t)W * (h / 2)) % 16) == 0) {
                    add_slots(p, K::LmSpread2, l, m, lm_spread2_blocks(w, h), in);
                    return;
                }
                plan_mode_lm_fast(p, K::LmFast2_128, 128, l, m, sh, in); return;
            case 4: plan_mode_lm_fast(p, K::LmFast4_64, 64, l, m, sh, in); return;
            case 5:
                // batches: the streaming kernel (one short wave per frame and band would not fill the chip for few frames)
                if (mode == 1 && !sh && batch(in) && spread5_shape(in, l, m)) { add_slots(p, K::LmSpread5, l, m, lm_spread5_blocks(w, h), in); return; }
                plan_mode_lm_fast(p, K::LmFast5_128, 128, l, m, sh, in); return;
            case 8: {
                const bool wide = lm_fast8_wide(W, h, mode, a_lm, in.a_stride, in.ori_stride, planes);
                plan_mode_lm_fast(p, wide ? K::LmFast8_80 : K::LmFast8_40, wide ? 80 : 40, l, m, sh, in); return;
            }
            default: break;
        }
    }
    // generic kernel (any T, any width).  Segment width: about 1024 linear-memory bytes per (band, segment), a multiple of 4 columns, and
    // few enough source bytes for LMK_MAX_LOADS loads per thread
    int seg = (1024 / (T * T)) & ~3;
    if (seg < 4) seg = 4;
    while (seg > 4 && (2 * T - 1) * (seg * T + T - 1) > LMK_MAX_LOADS * 256) seg -= 4;
    if (seg > W) seg = (W + 3) & ~3;
    const int pitch = (seg * T + T + 3) & ~3;
    PreStep& s = p.add(K::LinearMemories, l, m);
    s.gx = (u32)pre_ceil(W, seg); s.gy = (u32)(h / T); s.gz = (u32)in.n;
    s.param = seg; s.src_shift = sh; s.lds = (u32)(2048 + 2 * (size_t)(2 * T - 1) * pitch);
}

void plan_preprocess(const PreInputs& in, PrePlan& p) {
    const int M = in.M, L = in.L;
    p.n = 0; p.mask_step = -1;
    // few frames: one launch per dependency level, 5 launches instead of 14; batches: the same with the batch kernels (LM_TUNE_BATCH_PHASES)
    // when no other lane has work in flight -- alone on the chip the fused launches win, beside other lanes the separate ones interleave better.
    // Detector::match's masks apply to the quantised images: the fused routes quantise and spread in one go, so a call with a masked slot
    // takes the separate launches and the masks run between them.
    const bool few = in.n * in.weight <= in.phase_max_slots;
    const bool fuse_batch = in.batch_phases == 1 || (in.batch_phases == 2 && !in.others_busy);
    if (!in.masked && few && phases_shape(in)) { p.route = PreRoute::Phases; plan_phases(in, p); return; }
    if (!in.masked && !few && fuse_batch && batch_phases_shape(in)) { p.route = PreRoute::BatchPhases; plan_batch_phases(in, p); return; }
    p.route = PreRoute::Separate;
    const bool blur_pyr = L >= 2 && plan_blur_pyrdown(in, p);
    // two levels, level-0 blur + pyrDown done: the level-1 blur next, then BOTH levels' gradients in one grid
    bool grads_done = false;
    if (L == 2 && blur_pyr && half_size(in) && cgrad_levels_shape(in) && blur_streams(in, 1) && pick_blur(in, 1) != Blur::OneShot) {
        add_blur(in, 1, pick_blur(in, 1), p);
        plan_cgrad_levels(in, p);
        grads_done = true;
    }
    for (int l = 0; l < L; ++l) {
        if (l > 0 && !(l == 1 && blur_pyr)) plan_pyrdown(in, l, p);
        if (!grads_done) plan_color_quantize(in, l, l == 0 && blur_pyr, p);
        if (M == 2 && l == 0) plan_depth_quantize(in, p);
    }
    if (in.masked) { p.mask_step = p.n; p.add(K::MaskRules, 0, 0); p.add(K::MatchMasks, 0, 0); }
    if (M == 2 && L > 2) for (int l = 1; l < L; ++l) plan_nn_half(in, l, p);     // quant[l][1], l >= 1: DepthNormalPyramid::pyrDown
    for (int l = 0; l < L; ++l)
        for (int m = 0; m < M; ++m) plan_linear_memories(in, l, m, l == L - 1 ? in.planes : 0u, p);
}


#if defined(__x86_64__)
__attribute__((target("avx2"))) static void copy_stream_avx2(unsigned char* d, const unsigned char* s, size_t n) {
    const size_t head = (32 - (reinterpret_cast<uintptr_t>(d) & 31)) & 31;
    if (head) { std::memcpy(d, s, head); d += head; s += head; n -= head; }
    size_t i = 0;
    for (; i + 128 <= n; i += 128) {
        const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(s + i)), b = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(s + i + 32));
        const __m256i c = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(s + i + 64)), e = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(s + i + 96));
        _mm256_stream_si256(reinterpret_cast<__m256i*>(d + i), a); _mm256_stream_si256(reinterpret_cast<__m256i*>(d + i + 32), b);
        _mm256_stream_si256(reinterpret_cast<__m256i*>(d + i + 64), c); _mm256_stream_si256(reinterpret_cast<__m256i*>(d + i + 96), e);
    }
    for (; i + 32 <= n; i += 32) _mm256_stream_si256(reinterpret_cast<__m256i*>(d + i), _mm256_loadu_si256(reinterpret_cast<const __m256i*>(s + i)));
    if (i < n) std::memcpy(d + i, s + i, n - i);
}
#endif
void copy_stream(void* dst, const void* src, size_t n) {
#if defined(__x86_64__)
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2 && n >= 256) { copy_stream_avx2(static_cast<unsigned char*>(dst), static_cast<const unsigned char*>(src), n); return; }
#endif
    std::memcpy(dst, src, n);
}
void copy_stream_fence() {
#if defined(__x86_64__)
    _mm_sfence();
#endif
}

ShiftRect shift_rect(int w, int h, int ox, int oy) { return {std::max(ox, 0), std::min(w + ox, w), std::max(oy, 0), std::min(h + oy, h)}; }

void stage_rows_shifted(u8* staging, const u8* src, size_t stride, int w, int h, int px, int ox, int oy, int r0, int r1) {
    const size_t row_bytes = (size_t)w * px;
    const ShiftRect q = shift_rect(w, h, ox, oy);
    for (int y = r0; y < r1; ++y) {
        u8* row = staging + (size_t)y * row_bytes;
        if (y < q.y0 || y >= q.y1 || q.x1 <= q.x0) { std::memset(row, 0, row_bytes); continue; }
        if (q.x0 > 0) std::memset(row, 0, (size_t)q.x0 * px);
        copy_stream(row + (size_t)q.x0 * px, src + (size_t)(y - oy) * stride + (size_t)(q.x0 - ox) * px, (size_t)(q.x1 - q.x0) * px);     // non-temporal stores: the DMA engine reads this next
        if (q.x1 < w) std::memset(row + (size_t)q.x1 * px, 0, (size_t)(w - q.x1) * px);
    }
    copy_stream_fence();
}

// The tiles of the exported image that primitive `r` of a frame may touch: x tiles [*tx0, *tx1], y tiles [*ty0, *ty1]; false: none
static bool export_bin(const lmw::Rec& r, int w, int h, const ExportUndo& o, int* tx0, int* tx1, int* ty0, int* ty1) {
    const int fx0 = std::max(r.bx0, 0), fx1 = std::min(r.bx1, w - 1), fy0 = std::max(r.by0, 0), fy1 = std::min(r.by1, h - 1);
    if (fx0 > fx1 || fy0 > fy1) return false;
    const int ua = lmw::dest_x(fx0, w, o.flip_x, o.shift_x), ub = lmw::dest_x(fx1, w, o.flip_x, o.shift_x);
    const int u0 = std::max(std::min(ua, ub), 0), u1 = std::min(std::max(ua, ub), w - 1);
    const int v0 = std::max(lmw::dest_y(fy0, o.shift_y), 0), v1 = std::min(lmw::dest_y(fy1, o.shift_y), h - 1);
    if (u0 > u1 || v0 > v1) return false;
    *tx0 = u0 / EXPORT_TILE_W; *tx1 = u1 / EXPORT_TILE_W; *ty0 = v0 / EXPORT_TILE_H; *ty1 = v1 / EXPORT_TILE_H;
    return true;
}

bool plan_export(int w, int h, int n_frames, const ExportUndo* undo, const lm_draw_prim* prims, size_t n_prims, size_t max_entries, ExportPlan& p) {
    p = ExportPlan();
    p.tiles_x = (w + EXPORT_TILE_W - 1) / EXPORT_TILE_W; p.tiles_y = (h + EXPORT_TILE_H - 1) / EXPORT_TILE_H;
    const size_t tiles = (size_t)p.tiles_x * p.tiles_y, n_tiles = tiles * (size_t)n_frames;
    const ExportUndo none = {0, 0, 0};
    std::vector<lmw::Rec> recs(n_prims);
    std::vector<u32> count(n_tiles + 1, 0u);
    // pass 1: the records and the entries per tile
    for (size_t k = 0; k < n_prims; ++k) {
        const lm_draw_prim& q = prims[k];
        recs[k] = lmw::make_rec(q.kind, q.x0, q.y0, q.x1, q.y1, q.thickness, (u32)q.b | (u32)q.g << 8 | (u32)q.r << 16 | (u32)q.a << 24);
        int tx0, tx1, ty0, ty1;
        if (!export_bin(recs[k], w, h, undo ? undo[q.frame] : none, &tx0, &tx1, &ty0, &ty1)) continue;
        p.entries += (size_t)(tx1 - tx0 + 1) * (size_t)(ty1 - ty0 + 1);
        if (p.entries > max_entries) continue;      // (keep counting: the refusal names what the call needs)
        for (int ty = ty0; ty <= ty1; ++ty)
            for (int tx = tx0; tx <= tx1; ++tx) ++count[(size_t)q.frame * tiles + (size_t)ty * p.tiles_x + tx + 1];
    }
    if (p.entries > max_entries) return false;
    for (size_t t = 0; t < n_tiles; ++t) count[t + 1] += count[t];
    p.tile_off = count;
    p.idx.assign(p.entries, 0u);
    // pass 2: the indices, in list order (count[t] = the tile's next free entry)
    for (size_t k = 0; k < n_prims; ++k) {
        const lm_draw_prim& q = prims[k];
        int tx0, tx1, ty0, ty1;
        if (!export_bin(recs[k], w, h, undo ? undo[q.frame] : none, &tx0, &tx1, &ty0, &ty1)) continue;
        for (int ty = ty0; ty <= ty1; ++ty)
            for (int tx = tx0; tx <= tx1; ++tx) p.idx[count[(size_t)q.frame * tiles + (size_t)ty * p.tiles_x + tx]++] = (u32)k;
    }
    p.recs = std::move(recs);
    return true;
}
}  // namespace lmh
