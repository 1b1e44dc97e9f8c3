"""An independent numpy restatement of the oracle's match path from GIVEN quantised pyramids (oracle/linemod_oracle.cpp:
scan_template, match_template, orc_match_prepared), so that lists of masked frames -- which the oracle cannot produce, it calls
match without masks like the reference -- have an expected value: the quantised images ANDed with the mask pyramid, then this.

  a8-a10  spread, response maps (orc.spread, orc.response_maps), linearised here
  a11-a13 the scan at the coarsest level: u8 similarity sums per modality, their sum, the raw threshold rule of SURVEY.md A.7
  a14     local refinement down the levels: 16 x 16 patch around (2x + 1, 2y + 1) clamped to the border, first best position
  a15     sort under the total order of A.9, adjacent unique on (x, y, similarity, class)

Helper module (no test_ prefix): pytest does not collect it."""
import numpy as np

F32 = np.float32


def mask_pyramid(orc, mask0, levels):
    """Level l = level l-1 resized with INTER_NEAREST to half size (oracle.resize_nn_half), as pyrDown does with a mask."""
    out = [np.ascontiguousarray(mask0, np.uint8)]
    for _ in range(1, levels):
        out.append(orc.resize_nn_half(out[-1]))
    return out


def masked_pyramid(quant, masks_by_modality, levels, num_modalities, orc):
    """{(l, m): quantised image} -> the same with modality m's level-l image zeroed where its mask pyramid is zero (mask None: as is)."""
    out = {}
    for m in range(num_modalities):
        mk = masks_by_modality[m] if masks_by_modality is not None else None
        pyr = mask_pyramid(orc, mk, levels) if mk is not None else None
        for l in range(levels):
            q = quant[(l, m)]
            out[(l, m)] = q if pyr is None else np.where(pyr[l] != 0, q, 0).astype(np.uint8)
    return out


def split_bank(descs, features, levels, num_modalities):
    """(descs, features) in the lm_add_class layout -> per template a list over (level, modality) of (w, h, x, y, label)."""
    per = levels * num_modalities
    out, off = [], 0
    for t in range(len(descs) // per):
        tp = []
        for k in range(per):
            d = descs[t * per + k]
            nf = int(d["num_features"])
            f = features[off:off + nf]
            off += nf
            tp.append((int(d["width"]), int(d["height"]), f["x"].astype(np.int64), f["y"].astype(np.int64), f["label"].astype(np.int64)))
        out.append(tp)
    return out


def _cdiv(a, b):
    """C's integer division (truncation toward zero)."""
    q = abs(a) // b
    return q if a >= 0 else -q


class _Level:
    def __init__(self, orc, q, T, lut):
        h, w = q.shape
        self.w, self.h, self.T, self.W, self.H = w, h, T, w // T, h // T
        resp = orc.response_maps(orc.spread(q, T), lut)                    # [8][h][w]
        lm = resp.reshape(8, self.H, T, self.W, T).transpose(0, 2, 4, 1, 3).reshape(8, T * T * self.W * self.H)
        pad = np.zeros((8, self.W * self.H + 16 * self.W + 16), np.uint8)   # reads past an orientation's block are 0 (lm_read)
        self.lm = np.concatenate([lm, pad], axis=1)

    def index(self, x, y):
        T = self.T
        return ((y % T) * T + (x % T)) * self.W * self.H + (y // T) * self.W + (x // T)


def _scan(low, tmpl, threshold, ci, tid):
    """a11-a13 of one template: candidates as [x, y, similarity, template_id, class_idx] in row-major order."""
    total = np.zeros(low[0].W * low[0].H, np.int64)
    n = 0
    for lv, (tw, th, fx, fy, fl) in zip(low, tmpl):
        T, W, H = lv.T, lv.W, lv.H
        wf, hf = (tw - 1) // T + 1, (th - 1) // T + 1
        P = min(max((H - hf) * W + (W - wf) + 1, 0), W * H)
        sim = np.zeros(W * H, np.uint8)
        n += len(fx)
        for x, y, lab in zip(fx, fy, fl):
            if x < 0 or x >= lv.w or y < 0 or y >= lv.h:
                continue
            b = lv.index(int(x), int(y))
            sim[:P] += lv.lm[lab, b:b + P]                                     # u8 sums wrap like upstream's
        total += sim
    raw_thr = int(F32(2 * n) + (F32(threshold) / F32(100)) * F32(2 * n) + F32(0.5))
    T = low[0].T
    offset = T // 2 + (T % 2 - 1)
    out = []
    for k in np.flatnonzero(total > raw_thr):
        r, c = divmod(int(k), low[0].W)
        out.append([c * T + offset, r * T + offset, F32(F32(int(total[k])) * F32(100)) / F32(4 * n) + F32(0.5), tid, ci])
    return out


def _refine(levels_data, tp, cand, threshold, L, M, div=_cdiv):
    """a14 down the levels L-2 .. 0.  `div(x, T)` is the division that turns the clamped position into its patch origin: C's truncating
    one by default; tests pass another (floor) to show that a case tells the two apart."""
    for l in range(L - 2, -1, -1):
        lvs = levels_data[l]
        T, border = lvs[0].T, 8 * lvs[0].T
        offset = T // 2 + (T % 2 - 1)
        max_x = lvs[0].w - tp[l * M][0] - border
        max_y = lvs[0].h - tp[l * M][1] - border
        rr, cc = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
        kept = []
        for mm in cand:
            x = min(max(mm[0] * 2 + 1, border), max_x)
            y = min(max(mm[1] * 2 + 1, border), max_y)
            tot = np.zeros((16, 16), np.int64)
            nfs = 0
            off_x, off_y = (div(x, T) - 8) * T, (div(y, T) - 8) * T
            for m in range(M):
                lv = lvs[m]
                _, _, fx, fy, fl = tp[l * M + m]
                nfs += len(fx)
                loc = np.zeros((16, 16), np.uint8)
                for fx0, fy0, lab in zip(fx, fy, fl):
                    px, py = int(fx0) + off_x, int(fy0) + off_y
                    if px < 0 or py < 0 or px >= lv.w or py >= lv.h:
                        continue
                    loc += lv.lm[lab, lv.index(px, py) + rr * lv.W + cc]
                tot += loc
            best = int(tot.max())
            if best > 0:
                k = int(np.argmax(tot))                                         # first position of the row-major maximum
                br, bc = divmod(k, 16)
            else:
                br = bc = -1
            sim = F32(F32(best) * F32(100)) / F32(4 * nfs)
            if not sim < F32(threshold):
                kept.append([(div(x, T) - 8 + bc) * T + offset, (div(y, T) - 8 + br) * T + offset, sim, mm[3], mm[4]])
        cand = kept
    return cand


def match(orc, quant, classes, T, threshold, class_idx=-1, lut=None, match_dtype=None, div=_cdiv):
    """quant: {(level, modality): quantised image}; classes: list of (descs, features) per class (bank order); T: per level.
    Returns the oracle's list (oracle MATCH_DTYPE) for class `class_idx` (-1: all).  div: the refinement's division (see _refine)."""
    L = len(T)
    M = 1 + max(m for (_, m) in quant)
    levels_data = [[_Level(orc, quant[(l, m)], T[l], lut) for m in range(M)] for l in range(L)]
    out = []
    for ci, (descs, feats) in enumerate(classes):
        if class_idx >= 0 and ci != class_idx:
            continue
        for tid, tp in enumerate(split_bank(descs, feats, L, M)):
            cand = _scan(levels_data[L - 1], tp[(L - 1) * M:], threshold, ci, tid)
            out.extend(_refine(levels_data, tp, cand, threshold, L, M, div))
    out.sort(key=lambda r: (-float(r[2]), r[3], r[4], r[1], r[0]))
    uniq = []
    for r in out:
        if uniq and (uniq[-1][0], uniq[-1][1], uniq[-1][2], uniq[-1][4]) == (r[0], r[1], r[2], r[4]):
            continue
        uniq.append(r)
    res = np.zeros(len(uniq), match_dtype if match_dtype is not None else orc.MATCH_DTYPE)
    for i, r in enumerate(uniq):
        res[i] = (r[0], r[1], r[2], r[3], r[4])
    return res
