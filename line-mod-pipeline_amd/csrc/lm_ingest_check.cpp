// lm_ingest_check.cpp -- the descriptor check of the ingest family (lm_ingest_check.h): format word, colour or depth, null pointer, source
// size, window, chroma parity, row stride, plane stride, alignment, scale -- the first that fails wins -- and then the LmIngestImage.
#include "lm_ingest_check.h"

#include <cmath>

#include "lm_ingest_raw.h"

namespace lmc {

// LM_PIX_BGR8 .. LM_PIX_BAYER_BGGR8 (13 .. 15 name no format).  chroma: a chroma sample covers two columns (1: 4:2:2) or two columns and
// two rows (2: 4:2:0, and the chroma lies in a plane of its own) -- a source with half a pair at its edge has no chroma there.  The Bayer
// kinds: a 2 x 2 colour tile, so width and height are even like 4:2:0's, and a pixel reads its neighbours: the rows cover the whole source.
struct Format { int kind, bpp, swap_rb, is_depth, chroma; const char* name; };
static const Format FORMATS[] = {
    {LM_INGEST_PX3, 3, 0, 0, 0, "LM_PIX_BGR8"},           {LM_INGEST_PX3, 3, 1, 0, 0, "LM_PIX_RGB8"},
    {LM_INGEST_PX4, 4, 0, 0, 0, "LM_PIX_BGRA8"},          {LM_INGEST_PX4, 4, 1, 0, 0, "LM_PIX_RGBA8"},
    {LM_INGEST_PLANAR, 1, 0, 0, 0, "LM_PIX_BGR8_PLANAR"}, {LM_INGEST_PLANAR, 1, 1, 0, 0, "LM_PIX_RGB8_PLANAR"},
    {LM_INGEST_U16, 2, 0, 1, 0, "LM_PIX_DEPTH_U16"},      {LM_INGEST_F32, 4, 0, 1, 0, "LM_PIX_DEPTH_F32"},
    {LM_INGEST_GRAY8, 1, 0, 0, 0, "LM_PIX_GRAY8"},        {LM_INGEST_NV12, 1, 0, 0, 2, "LM_PIX_NV12"},
    {LM_INGEST_NV21, 1, 0, 0, 2, "LM_PIX_NV21"},          {LM_INGEST_YUY2, 2, 0, 0, 1, "LM_PIX_YUY2"},
    {LM_INGEST_UYVY, 2, 0, 0, 1, "LM_PIX_UYVY"},
    {0, 0, 0, 0, 0, nullptr},                             {0, 0, 0, 0, 0, nullptr},                             {0, 0, 0, 0, 0, nullptr},
    {LM_INGEST_BAYER_RGGB, 1, 0, 0, 0, "LM_PIX_BAYER_RGGB8"}, {LM_INGEST_BAYER_GRBG, 1, 0, 0, 0, "LM_PIX_BAYER_GRBG8"},
    {LM_INGEST_BAYER_GBRG, 1, 0, 0, 0, "LM_PIX_BAYER_GBRG8"}, {LM_INGEST_BAYER_BGGR, 1, 0, 0, 0, "LM_PIX_BAYER_BGGR8"}};
static_assert(sizeof(FORMATS) / sizeof(FORMATS[0]) == LM_PIX_BAYER_BGGR8 + 1, "one row per LM_PIX_* value up to the last format");
static_assert(LM_INGEST_BAYER_RGGB + 3 == LM_INGEST_BAYER_BGGR && LM_PIX_BAYER_RGGB8 + 3 == LM_PIX_BAYER_BGGR8, "format - 16 = kind - 10 = red_x | red_y << 1");

Geometry plain(const lm_config& c, Role role) {
    return {role, c.width, c.height, nullptr, 0, 0, nullptr, 0, 0, "window", c.width, false, "", SPANS, 0, 0, 0, 0};
}
Geometry rectified(const lm_config& c, const lm_rectification_desc& rect, Role role, bool whole) {
    return {role, c.width, c.height, "source camera", rect.source.width, rect.source.height, "ideal", rect.ideal.width, rect.ideal.height,
            "source", rect.source.width, whole, "rectification: ", DWORD, 0, 0, 0, 0};
}
Geometry raw_depth(const lm_config& c, const lm_registration_desc& reg, bool whole) {
    return {RAW_DEPTH, c.width, c.height, "registration's depth camera", reg.depth.width, reg.depth.height, "colour", reg.colour.width, reg.colour.height,
            "raw", reg.depth.width, whole, "", NEVER, 0, 0, 0, 0};
}

Geometry reduced(const lm_config& c, const lm_reduction_desc& red, Role role, bool whole) {
    const bool on = (red.apply & (role == COLOUR ? LM_REDUCE_COLOUR : LM_REDUCE_DEPTH)) != 0;
    Geometry g = plain(c, role);
    g.whole = whole; g.aligned = DWORD;
    if (on || whole) {
        g.row_name = "source"; g.prefix = "reduction: ";
        g.num_x = on ? red.num_x : 1; g.den_x = on ? red.den_x : 1; g.num_y = on ? red.num_y : 1; g.den_y = on ? red.den_y : 1;
    }
    return g;
}

Geometry rectified_reduced(const lm_config& c, const lm_rectification_desc& rect, const lm_reduction_desc& red, Role role, bool whole) {
    Geometry g = rectified(c, rect, role, whole);
    if (red.apply & (role == COLOUR ? LM_REDUCE_COLOUR : LM_REDUCE_DEPTH)) {
        g.bound_name = "reduced ideal";
        g.bound_w = (int)(((long long)rect.ideal.width * red.den_x) / red.num_x); g.bound_h = (int)(((long long)rect.ideal.height * red.den_y) / red.num_y);
    }
    return g;
}

static int gcd_of(int a, int b) { return b ? gcd_of(b, a % b) : a; }

std::string check_reduction(const lm_reduction_desc& in, lm_reduction_desc* out) {
    const int num[2] = {in.num_x, in.num_y}, den[2] = {in.den_x, in.den_y};
    int n[2], d[2];
    for (int k = 0; k < 2; ++k) {
        const std::string ax = k ? "_y " : "_x ", dn = "den" + ax + std::to_string(den[k]), nn = "num" + ax + std::to_string(num[k]);
        if (den[k] < 1 || den[k] > 16) return "reduction: " + dn + " lies outside 1 .. 16";
        if (num[k] < den[k]) return "reduction: " + nn + " is smaller than " + dn + ": an enlargement is not served";
        if (num[k] > 8 * den[k]) return "reduction: " + nn + " is larger than 8 " + dn;
        const int g = gcd_of(num[k], den[k]);
        n[k] = num[k] / g; d[k] = den[k] / g;
    }
    if (in.apply == 0) return "reduction: apply 0 names no image";
    if (in.apply & ~(LM_REDUCE_COLOUR | LM_REDUCE_DEPTH)) return "reduction: apply " + std::to_string(in.apply) + " has unknown bits";
    if (in.depth_rule != LM_REDUCE_DEPTH_NEAREST && in.depth_rule != LM_REDUCE_DEPTH_MIN_VALID) return "reduction: unknown depth_rule " + std::to_string(in.depth_rule);
    *out = {n[0], d[0], n[1], d[1], in.apply, in.depth_rule};
    return std::string();
}

std::string check_depth_call(const lm_config& c, bool registered, bool depth_given, bool* takes_depth) {
    *takes_depth = false;
    if (!keeps_depth(c)) {
        if (registered) return "lm_ingest_frames_registered needs an RGB-D detector: a colour-only detector holds no depth frame";
        return std::string();
    }
    *takes_depth = depth_given;
    return std::string();
}

static std::string size_words(int w, int h) { return std::to_string(w) + " x " + std::to_string(h); }

// LM_PIX_RAW | storage | pattern: LM_PIX_BAYER_RGGB10 .. LM_PIX_MONO12P
static std::string raw_name(int storage, int pattern) {
    static const char* const tiles[4] = {"RGGB", "GRBG", "GBRG", "BGGR"};
    static const char* const bits[6] = {"10", "12", "14", "16", "10P", "12P"};
    return (pattern == LM_RAW_MONO ? std::string("LM_PIX_MONO") : std::string("LM_PIX_BAYER_") + tiles[pattern]) + bits[storage];
}

// LM_PIX_FLOAT | element | layout: LM_PIX_BGR_F32 .. LM_PIX_GRAY_F16.  The layout is the 8-bit format's of the same memory order.
static int float_shape(int layout) {
    return layout <= LM_PIX_RGB8 ? LM_FLOAT_PX3 : layout <= LM_PIX_RGBA8 ? LM_FLOAT_PX4 : layout <= LM_PIX_RGB8_PLANAR ? LM_FLOAT_PLANAR
         : layout == LM_PIX_GRAY8 ? LM_FLOAT_GRAY : -1;
}
static std::string float_name(int half, int layout) {
    static const char* const order[9] = {"BGR", "RGB", "BGRA", "RGBA", "BGR", "RGB", "", "", "GRAY"};
    return std::string("LM_PIX_") + order[layout] + (half ? "_F16" : "_F32") + (float_shape(layout) == LM_FLOAT_PLANAR ? "_PLANAR" : "");
}

void process_bayer8(LmIngestImage* im) {
    if (lm_ingest_family(im->kind) != LM_INGEST_FAMILY_BAYER) return;
    im->kind = lm_raw_kind(LM_RAW_U8, im->kind - LM_INGEST_BAYER_RGGB);
    im->aligned = 0;
}

std::string check_image(const Geometry& g, const lm_image_desc& im, int frame, const lm_ingest_opts& o, LmIngestImage* out, int* matrix) {
    const auto refuse = [&](const char* prefix, const std::string& words) {
        return prefix + std::string(g.role == COLOUR ? "colour" : g.role == DEPTH ? "depth" : "raw depth") + " image of frame " + std::to_string(frame) + ": " + words;
    };
    // the matrix and range flags belong to the YUV formats alone; with any other bit set, or on another format, the value names no format
    const int flags = im.format >= 0 ? im.format & (LM_PIX_YUV_BT709 | LM_PIX_YUV_FULL) : 0, format = im.format - flags;
    // LM_PIX_RAW | storage | pattern and no other bit: a format of lm_ingest_raw.h, its row built here (bpp 0: rows are counted in bits)
    const bool raw = im.format >= 0 && (im.format & ~0xFF) == LM_PIX_RAW;
    const int storage = (im.format >> 4) & 15, pattern = im.format & 15;
    // LM_PIX_FLOAT | element | layout and no other bit: a format of lm_ingest_float.h, its row built here too
    const bool flt = im.format >= 0 && (im.format & ~0x1F) == LM_PIX_FLOAT;
    const int half = (im.format >> 4) & 1, es = half ? 2 : 4;
    if (raw ? storage > LM_RAW_P12 || pattern > LM_RAW_MONO
            : flt ? float_shape(pattern) < 0
            : format < LM_PIX_BGR8 || format > LM_PIX_BAYER_BGGR8 || !FORMATS[format].name || (flags && (format < LM_PIX_NV12 || format > LM_PIX_UYVY)))
        return refuse("", "unknown pixel format " + std::to_string(im.format));
    const std::string rname = raw ? raw_name(storage, pattern) : flt ? float_name(half, pattern) : std::string();
    const int fshape = flt ? float_shape(pattern) : 0;
    const Format rf = {raw ? lm_raw_kind(storage, pattern) : flt ? lm_float_kind(half, fshape) : 0,
                       flt ? es * (fshape == LM_FLOAT_PX3 ? 3 : fshape == LM_FLOAT_PX4 ? 4 : 1) : 0, flt ? pattern & 1 : 0, 0, 0, rname.c_str()};
    const Format& f = raw || flt ? rf : FORMATS[format];
    const bool bayer = raw ? pattern != LM_RAW_MONO : lm_ingest_family(f.kind) == LM_INGEST_FAMILY_BAYER;
    if (f.is_depth != (g.role != COLOUR)) return refuse("", f.name + std::string(f.is_depth ? " is a depth format" : " is a colour format"));
    if (!im.data) return refuse("", "null data pointer");
    if (g.source_name && (im.width != g.source_w || im.height != g.source_h))
        return refuse(g.prefix, "a " + size_words(im.width, im.height) + " image is not the " + g.source_name + " (" + size_words(g.source_w, g.source_h) + ")");
    if (g.den_x && (im.width < 1 || im.width > 32768 || im.height < 1 || im.height > 32768))
        return refuse(g.prefix, "width and height of a reduced source must lie in 1 .. 32768 (" + size_words(im.width, im.height) + ")");
    if (!g.whole && g.den_x) {
        const int bw = (int)(((long long)im.width * g.den_x) / g.num_x), bh = (int)(((long long)im.height * g.den_y) / g.num_y);
        if (im.crop_x < 0 || im.crop_y < 0 || (long long)im.crop_x + g.win_w > bw || (long long)im.crop_y + g.win_h > bh)
            return refuse(g.prefix, "window " + size_words(g.win_w, g.win_h) + " at (" + std::to_string(im.crop_x) + ", " + std::to_string(im.crop_y) +
                          ") lies outside the " + size_words(bw, bh) + " reduced geometry of a " + size_words(im.width, im.height) + " source");
    } else if (!g.whole) {
        // (the source itself as the bound: its size is the caller's word, so a negative one is refused here too)
        const int bw = g.bound_name ? g.bound_w : im.width, bh = g.bound_name ? g.bound_h : im.height;
        if (im.crop_x < 0 || im.crop_y < 0 || bw < 0 || bh < 0 || (long long)im.crop_x + g.win_w > bw || (long long)im.crop_y + g.win_h > bh) {
            const std::string window = "window " + size_words(g.win_w, g.win_h) + " at (" + std::to_string(im.crop_x) + ", " + std::to_string(im.crop_y) + ")";
            if (g.bound_name) return refuse(g.prefix, window + " lies outside the " + size_words(bw, bh) + " " + g.bound_name + " geometry");
            return refuse(g.prefix, "0 <= roi.x && roi.x + roi.width <= m.cols && 0 <= roi.y && roi.y + roi.height <= m.rows failed: " + window + " in a " +
                          size_words(bw, bh) + " source");
        }
    }
    if ((f.chroma == 2 || bayer) && (im.width % 2 || im.height % 2)) return refuse("", std::string("width and height of a ") + f.name + " source must be even");
    if (f.chroma == 1 && im.width % 2) return refuse("", std::string("width of a ") + f.name + " source must be even");
    const bool planes = f.kind == LM_INGEST_PLANAR || f.chroma == 2 || (flt && fshape == LM_FLOAT_PLANAR);
    // (a Bayer pixel's neighbours lie outside the window: its rows must hold the source's width, which is no smaller than the window's)
    // (a raw row, Bayer or mono: the source's width in whole u16 samples or in ceil(width * N / 8) packed bytes)
    const long long row_px = g.den_x || ((bayer || raw) && im.width > g.row_w) ? im.width : g.row_w;
    if (im.row_stride < (raw ? (row_px * lm_raw_row_bits(storage) + 7) / 8 : row_px * f.bpp)) return refuse(g.prefix, std::string("row_stride smaller than a ") + g.row_name + " row");
    if (planes && im.plane_stride <= 0) return refuse("", "plane_stride must be positive");
    if (f.is_depth) {
        if (reinterpret_cast<uintptr_t>(im.data) % f.bpp || im.row_stride % f.bpp)
            return refuse("", std::string("data and row_stride of a ") + (f.bpp == 2 ? "u16" : "f32") + " source must be multiples of " + std::to_string(f.bpp));
        if (f.kind == LM_INGEST_F32 && !(std::isfinite(im.scale) && im.scale > 0.0f)) return refuse("", "scale must be finite and positive");
    }
    if (flt) {
        const std::string who = std::string(half ? "f16" : "f32") + " source must be ";
        if (reinterpret_cast<uintptr_t>(im.data) % es || im.row_stride % es) return refuse("", "data and row_stride of a " + who + "multiples of " + std::to_string(es));
        if (planes && im.plane_stride % es) return refuse("", "plane_stride of a " + who + "a multiple of " + std::to_string(es));
        if (!(std::isfinite(im.scale) && im.scale > 0.0f)) return refuse("", "scale must be finite and positive");
    }
    if (raw && storage < LM_RAW_P10 && (reinterpret_cast<uintptr_t>(im.data) % 2 || im.row_stride % 2))
        return refuse("", "data and row_stride of a u16 source must be multiples of 2");
    *out = LmIngestImage();
    out->data = static_cast<const uint8_t*>(im.data);
    out->row_stride = im.row_stride; out->plane_stride = planes ? im.plane_stride : 0;
    out->crop_x = g.whole ? 0 : im.crop_x; out->crop_y = g.whole ? 0 : im.crop_y;
    out->kind = f.kind; out->swap_rb = f.swap_rb;
    out->src_w = im.width; out->src_h = im.height;
    out->scale = im.scale;
    if (matrix) *matrix = flags >> 8;
    if (raw) return std::string();          // (aligned stays 0: lm_ingest_raw.h loads every span by the general path)
    if (g.aligned == SPANS) {
        // the fast path: every lane's span starts on a 16-byte boundary.  A lane's first source column is crop_x + x0 - shift_x, or
        // crop_x + W - 16 - x0 + shift_x when mirrored, x0 a multiple of 16.
        const long long col0 = (long long)im.crop_x + (o.flip_x ? g.win_w - 16 + o.shift_x : -o.shift_x);
        out->aligned = lmi::spans_aligned(reinterpret_cast<uintptr_t>(im.data), im.row_stride, out->plane_stride, col0, f.bpp);
    } else if (g.aligned == DWORD) {
        out->aligned = f.kind == LM_INGEST_PX4 && reinterpret_cast<uintptr_t>(im.data) % 4 == 0 && im.row_stride % 4 == 0;
    }
    return std::string();
}

}  // namespace lmc
