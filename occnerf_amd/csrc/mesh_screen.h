// What the kernels that look through a frame's camera share (mesh_raster.hip, mesh_texture.hip, mesh_normal.hip; DESIGN.md sections
// 7j, 7o, 7p, 7q): the pinhole camera with its vertex rule and its three limits (mesh_texture.hip's triangle weights take the
// camera and the limits and state the rule again without its coordinates; DESIGN.md section 7o says why), the key of an empty
// pixel, the image-size test, the background, the byte a weighted sum of bytes is stored as, and the winner of a pixel -- the
// triangle its key names, as the textured and the lit resolve see it.  mesh_raster.hip's own mesh_resolve_kernel states its
// screen-space triangle itself; see DESIGN.md section 7o for why.  fp64 with + - * / rint and comparisons only, one rounding per
// operator in the order of tests/mesh_raster_restatement.py.
#pragma once

#include "common.h"

namespace occ {

constexpr unsigned long long kRasterEmpty = ~0ull;        // the key of a pixel no triangle covers
constexpr double kScreenNear = 1e-3;
constexpr double kScreenFar = 1048576.0;                  // 2^20
constexpr double kScreenGuard = 4194304.0;                // 2^22 fixed-point units

// H and W in 1..kRasterMaxSide and at most 2^28 pixels (mesh_raster.hip, beside the rasteriser's other limits).
bool raster_size_ok(int32_t H, int32_t W);

struct RasterBg {
    uint8_t c[3];
};

// rint, then clamped to a byte (a NaN gives 0).
__device__ __forceinline__ uint8_t raster_byte(double s) {
    const double r = rint(s);
    return (uint8_t)(r > 0.0 ? (r < 255.0 ? r : 255.0) : 0.0);
}

__device__ __forceinline__ double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

struct ScreenCamera {
    double fx, fy, cx, cy;
    double R[9], t[3];
};

// K 3x3 without skew and E = [R | t] 4x4, row-major on the host.
inline ScreenCamera screen_camera(const double *h_K, const double *h_E) {
    ScreenCamera cam;
    cam.fx = h_K[0], cam.fy = h_K[4], cam.cx = h_K[2], cam.cy = h_K[5];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) cam.R[r * 3 + c] = h_E[r * 4 + c];
        cam.t[r] = h_E[r * 4 + 3];
    }
    return cam;
}

// The vertex rule: p -> its camera-space point c and its unrounded coordinates (a, b) in 1/256 pixel; the flag comes back: 1
// nearer than kScreenNear (or NaN), 2 past the guard band or kScreenFar, 0 kept.
__device__ __forceinline__ int screen_vertex(const ScreenCamera &cam, const float *__restrict__ p, double c[3], double &a, double &b) {
    const double p0 = (double)p[0], p1 = (double)p[1], p2 = (double)p[2];
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = ((cam.R[k * 3] * p0 + cam.R[k * 3 + 1] * p1) + cam.R[k * 3 + 2] * p2) + cam.t[k];
    a = 256.0 * (cam.fx * (c[0] / c[2]) + cam.cx);
    b = 256.0 * (cam.fy * (c[1] / c[2]) + cam.cy);
    int flag = 0;
    if (!(c[2] >= kScreenNear)) flag = 1;
    else if (!(fabs(a) <= kScreenGuard && fabs(b) <= kScreenGuard && c[2] <= kScreenFar)) flag = 2;
    return flag;
}

struct ScreenWinner {
    int64_t col, row;          // the pixel
    int64_t t;                 // the triangle
    int32_t v0, v1, v2;        // its vertices, each in [0, V)
    double w0, w1, w2;         // the perspective-correct weights of the pixel's sample, in the face's own order
};

// The winner of pixel pix of an image W wide from its key; false: the background (an empty key, an index out of range, no area,
// a flagged vertex).  (a, b, c) is the triangle as mesh_raster.hip's raster_setup orders it, vertices 1 and 2 exchanged when the
// area is negative; e_k, q_k and the weights are that triangle's, as mesh_resolve_kernel forms them.  The pixel's column and row
// are formed for a winner only: a 64-bit division the background does not pay for.
__device__ __forceinline__ bool screen_winner(unsigned long long key, const int32_t *__restrict__ faces, int64_t T, int64_t V,
                                              const int32_t *__restrict__ xy, const double *__restrict__ z, int64_t pix, int W,
                                              ScreenWinner &s) {
    const int64_t t = (int64_t)(key & 0xFFFFFFFFull);
    if (key != kRasterEmpty && t < T) {
        const int32_t v0 = faces[t * 3], v1 = faces[t * 3 + 1], v2 = faces[t * 3 + 2];
        if (v0 >= 0 && v0 < V && v1 >= 0 && v1 < V && v2 >= 0 && v2 < V) {
            const int64_t X0 = xy[(int64_t)v0 * 2], Y0 = xy[(int64_t)v0 * 2 + 1];
            const int64_t X1 = xy[(int64_t)v1 * 2], Y1 = xy[(int64_t)v1 * 2 + 1];
            const int64_t X2 = xy[(int64_t)v2 * 2], Y2 = xy[(int64_t)v2 * 2 + 1];
            const double z0 = z[v0], z1 = z[v1], z2 = z[v2];
            const int64_t As = (X1 - X0) * (Y2 - Y0) - (Y1 - Y0) * (X2 - X0);
            if (As != 0 && z0 > 0.0 && z1 > 0.0 && z2 > 0.0) {           // (a flagged vertex has z = 0)
                const bool flip = As < 0;
                const int64_t col = pix % W, row = pix / W;
                const int64_t px = 256ll * col, py = 256ll * row;
                const int64_t Xa = X0, Ya = Y0;
                const int64_t Xb = flip ? X2 : X1, Yb = flip ? Y2 : Y1, Xc = flip ? X1 : X2, Yc = flip ? Y1 : Y2;
                const double zb = flip ? z2 : z1, zc = flip ? z1 : z2;
                const int64_t e0 = (Xc - Xb) * (py - Yb) - (Yc - Yb) * (px - Xb);
                const int64_t e1 = (Xa - Xc) * (py - Yc) - (Ya - Yc) * (px - Xc);
                const int64_t e2 = (Xb - Xa) * (py - Ya) - (Yb - Ya) * (px - Xa);
                const double a = (double)(flip ? -As : As);
                const double q0 = ((double)e0 / a) / z0, q1 = ((double)e1 / a) / zb, q2 = ((double)e2 / a) / zc;
                const double iz = (q0 + q1) + q2;
                const double wb = q1 / iz, wc = q2 / iz;
                s.col = col, s.row = row, s.t = t, s.v0 = v0, s.v1 = v1, s.v2 = v2;
                s.w0 = q0 / iz, s.w1 = flip ? wc : wb, s.w2 = flip ? wb : wc;       // back in the face's own order
                return true;
            }
        }
    }
    return false;
}

}  // namespace occ
