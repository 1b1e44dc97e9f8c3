// lm_export_check.cpp -- the checks of lm_export_frames (lm_export_check.h): the frame, a destination descriptor -- format word, served
// or not, null pointer, window, NV12 parity, row stride, plane stride, a float destination's alignment and scale; the first that fails wins -- the overlap of two destinations, and
// a primitive.
#include "lm_export_check.h"

#include <cmath>

#include "lm_draw.h"

namespace lmc {

static std::string size_words(int w, int h) { return std::to_string(w) + " x " + std::to_string(h); }

std::string check_export_counts(bool dst_null, int n_slots, bool prims_null, size_t n_prims) {
    if (dst_null || n_slots <= 0) return "export: bad argument: a null dst or n_slots <= 0";
    if (prims_null && n_prims > 0) return "export: bad argument: null prims with n_prims > 0";
    if (n_prims > (size_t)EXPORT_MAX_PRIMS) return "export: " + std::to_string(n_prims) + " primitives exceed 65536";
    return std::string();
}

std::string check_export_frame(int w, int h) {
    if (w > lmw::FRAME_MAX || h > lmw::FRAME_MAX) return "export: a " + size_words(w, h) + " frame is wider or higher than 8192";
    if (w < 16 || h < 1 || w % 16) return "export: lm_export_frames needs a frame width that is a multiple of 16";
    return std::string();
}

// LM_PIX_BGR8 .. LM_PIX_RGB8_PLANAR (row k = format k) and LM_PIX_NV12 are served, and the float formats with the layouts of the first six
struct Served { int format, kind, bpp, swap_rb; const char* name; };
static const Served SERVED[] = {
    {LM_PIX_BGR8, LM_EXPORT_PX3, 3, 0, "LM_PIX_BGR8"},           {LM_PIX_RGB8, LM_EXPORT_PX3, 3, 1, "LM_PIX_RGB8"},
    {LM_PIX_BGRA8, LM_EXPORT_PX4, 4, 0, "LM_PIX_BGRA8"},         {LM_PIX_RGBA8, LM_EXPORT_PX4, 4, 1, "LM_PIX_RGBA8"},
    {LM_PIX_BGR8_PLANAR, LM_EXPORT_PLANAR, 1, 0, "LM_PIX_BGR8_PLANAR"}, {LM_PIX_RGB8_PLANAR, LM_EXPORT_PLANAR, 1, 1, "LM_PIX_RGB8_PLANAR"},
    {LM_PIX_NV12, LM_EXPORT_NV12, 1, 0, "LM_PIX_NV12"}};

static const char* source_only_name(int format) {
    switch (format) {
        case LM_PIX_GRAY8: return "LM_PIX_GRAY8";
        case LM_PIX_NV21: return "LM_PIX_NV21";
        case LM_PIX_YUY2: return "LM_PIX_YUY2";
        case LM_PIX_UYVY: return "LM_PIX_UYVY";
        case LM_PIX_BAYER_RGGB8: return "LM_PIX_BAYER_RGGB8";
        case LM_PIX_BAYER_GRBG8: return "LM_PIX_BAYER_GRBG8";
        case LM_PIX_BAYER_GBRG8: return "LM_PIX_BAYER_GBRG8";
        case LM_PIX_BAYER_BGGR8: return "LM_PIX_BAYER_BGGR8";
        default: return nullptr;
    }
}

std::string check_export_image(int w, int h, const lm_image_desc& im, int frame, LmExportImage* out) {
    const auto refuse = [&](const std::string& words) { return "destination image of frame " + std::to_string(frame) + ": " + words; };
    // the matrix and range flags belong to NV12 alone; with any other bit set, or on another format, the value names no format
    const int flags = im.format >= 0 ? im.format & (LM_PIX_YUV_BT709 | LM_PIX_YUV_FULL) : 0, format = im.format - flags;
    const Served* f = nullptr;
    for (const Served& s : SERVED) if (s.format == format) f = &s;
    if (f && flags && f->kind != LM_EXPORT_NV12) f = nullptr;
    // LM_PIX_FLOAT | element | layout and no other bit: the layouts of the six 8-bit RGB formats are destinations, with es-byte elements
    const bool flt = im.format >= 0 && (im.format & ~0x1F) == LM_PIX_FLOAT;
    const int es = flt ? ((im.format & LM_PIX_FLOAT_F16) ? 2 : 4) : 0, layout = im.format & 15;
    Served ff = {im.format, 0, 0, 0, nullptr};
    if (flt && layout <= LM_PIX_RGB8_PLANAR) {
        ff.kind = SERVED[layout].kind; ff.bpp = SERVED[layout].bpp * es; ff.swap_rb = SERVED[layout].swap_rb;
        f = &ff;
    }
    if (!f) {
        if (!flags && (format == LM_PIX_DEPTH_U16 || format == LM_PIX_DEPTH_F32))
            return refuse(std::string(format == LM_PIX_DEPTH_U16 ? "LM_PIX_DEPTH_U16" : "LM_PIX_DEPTH_F32") + " is a depth format: depth export is not served");
        if (flt && layout == LM_PIX_GRAY8) return refuse(std::string(es == 2 ? "LM_PIX_GRAY_F16" : "LM_PIX_GRAY_F32") + " is a source format: not served as a destination");
        const bool raw = im.format >= 0 && (im.format & ~0xFF) == LM_PIX_RAW && ((im.format >> 4) & 15) <= 5 && (im.format & 15) <= 4;
        const char* name = raw ? "a raw format" : (format == LM_PIX_GRAY8 || format >= LM_PIX_BAYER_RGGB8) && flags ? nullptr : source_only_name(format);
        if (name) return refuse(std::string(name) + " is a source format: not served as a destination");
        return refuse("unknown pixel format " + std::to_string(im.format));
    }
    if (!im.data) return refuse("null data pointer");
    if (im.crop_x < 0 || im.crop_y < 0 || im.width < 0 || im.height < 0 || (long long)im.crop_x + w > im.width || (long long)im.crop_y + h > im.height)
        return refuse("window " + size_words(w, h) + " at (" + std::to_string(im.crop_x) + ", " + std::to_string(im.crop_y) + ") lies outside the " +
                      size_words(im.width, im.height) + " surface");
    if (f->kind == LM_EXPORT_NV12 && ((im.crop_x | im.crop_y | im.width | im.height | h) & 1))
        return refuse("crop_x, crop_y, width and height of a LM_PIX_NV12 destination, and the frame's height, must be even");
    if (im.row_stride < (long long)im.width * f->bpp) return refuse("row_stride smaller than a surface row");
    const bool planes = f->kind == LM_EXPORT_PLANAR || f->kind == LM_EXPORT_NV12;
    if (planes && im.plane_stride <= 0) return refuse("plane_stride must be positive");
    if (flt) {
        const std::string who = std::string(es == 2 ? "f16" : "f32") + " source must be ";
        if (reinterpret_cast<uintptr_t>(im.data) % es || im.row_stride % es) return refuse("data and row_stride of a " + who + "multiples of " + std::to_string(es));
        if (planes && im.plane_stride % es) return refuse("plane_stride of a " + who + "a multiple of " + std::to_string(es));
        if (!(std::isfinite(im.scale) && im.scale > 0.0f)) return refuse("scale must be finite and positive");
    }
    *out = LmExportImage();
    out->data = static_cast<uint8_t*>(const_cast<void*>(im.data));
    out->row_stride = im.row_stride; out->plane_stride = planes ? im.plane_stride : 0;
    out->crop_x = im.crop_x; out->crop_y = im.crop_y;
    out->kind = f->kind; out->swap_rb = f->swap_rb; out->matrix = flags >> 8;
    out->es = es; out->scale = flt ? im.scale : 0.0f;
    return std::string();
}

// the window's byte ranges [first, last] per plane
struct Range { uintptr_t first, last; };
static int ranges_of(int w, int h, const LmExportImage& e, Range (&r)[3]) {
    const uintptr_t base = reinterpret_cast<uintptr_t>(e.data);
    const auto plane = [&](long long off, int bpp, int y0, int rows) {
        Range g;
        g.first = base + (uintptr_t)(off + (long long)y0 * e.row_stride + (long long)e.crop_x * bpp);
        g.last = base + (uintptr_t)(off + (long long)(y0 + rows - 1) * e.row_stride + (long long)(e.crop_x + w) * bpp - 1);
        return g;
    };
    const int el = e.es ? e.es : 1;        // (a float destination's pixels are counted in element bytes)
    if (e.kind == LM_EXPORT_PX3 || e.kind == LM_EXPORT_PX4) { r[0] = plane(0, (e.kind == LM_EXPORT_PX3 ? 3 : 4) * el, e.crop_y, h); return 1; }
    if (e.kind == LM_EXPORT_PLANAR) { for (int k = 0; k < 3; ++k) r[k] = plane(k * e.plane_stride, el, e.crop_y, h); return 3; }
    r[0] = plane(0, 1, e.crop_y, h);
    r[1] = plane(e.plane_stride, 1, e.crop_y / 2, h / 2);
    return 2;
}

std::string check_export_overlap(int w, int h, const LmExportImage* images, int n) {
    for (int i = 0; i < n; ++i) {
        Range a[3];
        const int na = ranges_of(w, h, images[i], a);
        for (int j = i + 1; j < n; ++j) {
            Range b[3];
            const int nb = ranges_of(w, h, images[j], b);
            for (int p = 0; p < na; ++p)
                for (int q = 0; q < nb; ++q)
                    if (a[p].first <= b[q].last && b[q].first <= a[p].last)
                        return "destination images of frames " + std::to_string(i) + " and " + std::to_string(j) + " overlap in memory";
        }
    }
    return std::string();
}

std::string check_export_prim(const lm_draw_prim& p, size_t k, int n_frames) {
    const auto refuse = [&](const std::string& words) { return "primitive " + std::to_string(k) + ": " + words; };
    if (p.kind != LM_DRAW_RING && p.kind != LM_DRAW_SEGMENT && p.kind != LM_DRAW_BOX) return refuse("unknown kind " + std::to_string(p.kind));
    if (p.frame < 0 || p.frame >= n_frames) return refuse("frame " + std::to_string(p.frame) + " lies outside 0 .. " + std::to_string(n_frames - 1));
    const bool ring = p.kind == LM_DRAW_RING;
    const int xy[4] = {p.x0, p.y0, p.x1, p.y1};
    for (int c = 0; c < (ring ? 2 : 4); ++c)
        if (xy[c] < lmw::COORD_MIN || xy[c] > lmw::COORD_MAX) return refuse("coordinate " + std::to_string(xy[c]) + " lies outside -8192 .. 8191");
    if (p.thickness < 1 || p.thickness > lmw::THICK_MAX) return refuse("thickness " + std::to_string(p.thickness) + " lies outside 1 .. 64");
    if (ring && (p.y1 != 0 || p.x1 < 0 || p.x1 > lmw::COORD_MAX)) return refuse("a ring needs y1 == 0 and a radius in 0 .. 8191");
    if (p.kind == LM_DRAW_BOX && (p.x0 > p.x1 || p.y0 > p.y1)) return refuse("inverted box");
    return std::string();
}

}  // namespace lmc
