// lm_register.h -- the arithmetic of the depth registration (lm_k_register.hip; the rule is written out in
// include/linemod_hip.h) as functions the host can run too: what ONE raw depth pixel becomes on the colour camera (project), and the ray
// table of a pinhole + Brown-Conrady depth camera (build_rays, host only).  project is IEEE single precision, every operation rounded on
// its own in the order written: the sources that include this header are compiled with -ffp-contract=off, and `/` is the correctly
// rounded division.  tests/cpp/register_host.cpp drives exactly this code with g++ under ASan / UBSan.  No GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LMR_FN __host__ __device__ __forceinline__
#else
#define LMR_FN inline
#endif

namespace lmr {

// the colour side of a registration: P_colour = R * P_depth + t (millimetres), then the colour lens
struct Rig {
    float r[9], t[3];                           // R row-major
    float fx, fy, cx, cy, k1, k2, p1, p2, k3;   // the colour camera
};

// What a depth pixel contributes: m (1 .. 65535 millimetres) to the colour pixels around (u, v), unless it is dropped.  u and v are
// finite whole numbers IN FLOAT: they may lie far outside the int range, so the caller compares them as floats before it converts.
struct Hit { int dropped; float u, v; uint32_t m; };

LMR_FN bool finite(float x) { return __builtin_isfinite(x); }

// t: the pixel's depth in millimetres (v * scale of a float source, (float)v of a u16 one); (rx, ry): its ray
LMR_FN Hit project(const Rig& g, float rx, float ry, float t) {
    Hit h;
    h.dropped = 1; h.u = 0.0f; h.v = 0.0f; h.m = 0u;
    if (!(finite(t) && t > 0.0f)) return h;
    const float X = rx * t, Y = ry * t;
    const float Xc = ((g.r[0] * X + g.r[1] * Y) + g.r[2] * t) + g.t[0];
    const float Yc = ((g.r[3] * X + g.r[4] * Y) + g.r[5] * t) + g.t[1];
    const float Zc = ((g.r[6] * X + g.r[7] * Y) + g.r[8] * t) + g.t[2];
    if (!(finite(Zc) && Zc > 0.0f)) return h;
    const float a = Xc / Zc, b = Yc / Zc;
    const float r2 = a * a + b * b;
    const float rad = 1.0f + r2 * (g.k1 + r2 * (g.k2 + r2 * g.k3));
    const float ad = a * rad + ((2.0f * g.p1) * (a * b) + g.p2 * (r2 + 2.0f * (a * a)));
    const float bd = b * rad + (g.p1 * (r2 + 2.0f * (b * b)) + (2.0f * g.p2) * (a * b));
    const float xf = g.fx * ad + g.cx, yf = g.fy * bd + g.cy;
    const float u = __builtin_floorf(xf + 0.5f), v = __builtin_floorf(yf + 0.5f);
    if (!(finite(u) && finite(v))) return h;
    const float zr = __builtin_rintf(Zc);          // ties to even
    const float m = zr < 65535.0f ? zr : 65535.0f;
    if (m < 1.0f) return h;
    h.dropped = 0; h.u = u; h.v = v; h.m = (uint32_t)m;
    return h;
}

// The ray table of a pinhole + Brown-Conrady camera, rays[2 * (j * w + i)] = rx, [.. + 1] = ry of pixel (i, j): the distorted normalised
// coordinate ((i - cx) / fx, (j - cy) / fy) pushed through the inverse Brown model by LMR_RAY_ITERATIONS rounds of the fixed-point
// iteration x <- (xd - tangential(x)) / radial(x), all in double, rounded to float once.  With the five coefficients zero radial is 1 and
// tangential 0 in every round: the result is the rounded quotient itself.
enum { LMR_RAY_ITERATIONS = 20 };
inline void build_rays(double fx, double fy, double cx, double cy, double k1, double k2, double p1, double p2, double k3, int w, int h, float* rays) {
    for (int j = 0; j < h; ++j)
        for (int i = 0; i < w; ++i) {
            const double xd = ((double)i - cx) / fx, yd = ((double)j - cy) / fy;
            double x = xd, y = yd;
            for (int it = 0; it < LMR_RAY_ITERATIONS; ++it) {
                const double r2 = x * x + y * y;
                const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
                const double dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x), dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
                x = (xd - dx) / rad; y = (yd - dy) / rad;
            }
            float* o = rays + 2 * ((size_t)j * (size_t)w + (size_t)i);
            o[0] = (float)x; o[1] = (float)y;
        }
}

}  // namespace lmr
