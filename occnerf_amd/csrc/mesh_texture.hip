// The texture of the exported mesh (occnerf_amd/mesh.py bake_texture / export_texture): a per-triangle atlas.
// Triangles 2c and 2c + 1 share the n x n cell c; the even one owns the texels i + j <= n - 2 of the cell, the odd one those of
// the mirrored frame i' = n - 1 - i, j' = n - 1 - j; every triangle owns P = n (n - 1) / 2 texels, numbered by ascending j',
// then ascending i'; texel (i', j') stands for the barycentric numerators (m - i' - j', i', j') over m = n - 3.
//
//   mesh_texel_points       one thread per texel: its canonical point, the colour field's query;
//   mesh_texture_fill       one thread per texel: the queried colour as a byte at its place in the atlas;
//   mesh_resolve_textured   one thread per pixel of mesh_raster's keys: the winner's perspective-correct weights as
//                           mesh_raster.hip's resolve forms them, then four taps of the atlas, all of them the winner's own texels.
//
// fp64 on the float32 inputs with + - * / floor rint and comparisons only, one rounding per operator in the order of
// tests/mesh_texture_restatement.py (the tree is built with -ffp-contract=off); the fill's product is the float32 one of
// image.to_8b_image.  No atomics; every output is a pure function of the inputs: the same bytes on every run.  Every index read
// from faces or from a key is checked before it is used as an address, and every atlas address lies inside the C x R cells the
// entry has checked against the atlas' size.  The empty key, the image-size test, the background and the byte store are
// mesh_screen.h's, shared with mesh_raster.hip's resolve.
#include "common.h"
#include "mesh_screen.h"

namespace occ {

constexpr int kTexThreads = 256;
constexpr int kTexMinCell = 4;
constexpr int kTexMaxCell = 64;
constexpr int kTexMaxSide = 16384;

// Texel k of a triangle -> (i', j') in its own frame: row j' holds the n - 1 - j' texels i' = 0 .. n - 2 - j'.
__device__ __forceinline__ void texel_of(int k, int n, int &i, int &j) {
    int row = n - 1;
    j = 0;
    while (k >= row) {              // at most n - 2 <= 62 steps
        k -= row;
        row--;
        j++;
    }
    i = k;
}

// (column, row) in the atlas of texel (i', j') of triangle t.
__device__ __forceinline__ void atlas_of(int64_t t, int i, int j, int n, int C, int &x, int &y) {
    const int64_t c = t >> 1;
    const bool odd = (t & 1) != 0;
    x = (int)(c % C) * n + (odd ? n - 1 - i : i);
    y = (int)(c / C) * n + (odd ? n - 1 - j : j);
}

__global__ __launch_bounds__(kTexThreads) void mesh_texel_points_kernel(const float *__restrict__ verts, int64_t V,
                                                                        const int32_t *__restrict__ faces, int64_t T, int n, int P,
                                                                        float *__restrict__ pts, int32_t *__restrict__ status) {
    const int64_t g = (int64_t)blockIdx.x * kTexThreads + threadIdx.x;
    if (g >= T * P) return;
    const int64_t t = g / P;
    int i, j;
    texel_of((int)(g - t * P), n, i, j);
    const int32_t v0 = faces[t * 3], v1 = faces[t * 3 + 1], v2 = faces[t * 3 + 2];
    if (v0 < 0 || v0 >= V || v1 < 0 || v1 >= V || v2 < 0 || v2 >= V) {
        const float nan = __uint_as_float(0x7FC00000u);
        pts[g * 3] = nan, pts[g * 3 + 1] = nan, pts[g * 3 + 2] = nan;
        status[0] = 1;                          // every thread that gets here stores the same value
        return;
    }
    const int m = n - 3;
    const double b0 = (double)(m - i - j), b1 = (double)i, b2 = (double)j, dm = (double)m;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double s = (b0 * (double)verts[(int64_t)v0 * 3 + c] + b1 * (double)verts[(int64_t)v1 * 3 + c]) +
                         b2 * (double)verts[(int64_t)v2 * 3 + c];
        pts[g * 3 + c] = (float)(s / dm);
    }
}

__global__ __launch_bounds__(kTexThreads) void mesh_texture_fill_kernel(const float *__restrict__ rgb, int64_t T, int n, int P, int C,
                                                                        int W, uint8_t *__restrict__ atlas) {
    const int64_t g = (int64_t)blockIdx.x * kTexThreads + threadIdx.x;
    if (g >= T * P) return;
    const int64_t t = g / P;
    int i, j, x, y;
    texel_of((int)(g - t * P), n, i, j);
    atlas_of(t, i, j, n, C, x, y);
    uint8_t *out = atlas + ((int64_t)y * W + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float v = rgb[g * 3 + c];
        const float u = v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f;          // (a NaN fails the first comparison: 0)
        out[c] = (uint8_t)(int)(255.0f * u);
    }
}

__global__ __launch_bounds__(kTexThreads) void mesh_resolve_textured_kernel(
    const unsigned long long *__restrict__ keys, const int32_t *__restrict__ faces, int64_t T, int64_t V,
    const int32_t *__restrict__ xy, const double *__restrict__ z, int H, int W, const uint8_t *__restrict__ atlas, int aW, int n,
    int C, RasterBg bg, uint8_t *__restrict__ rgb) {
    const int64_t pix = (int64_t)blockIdx.x * kTexThreads + threadIdx.x;
    if (pix >= (int64_t)H * W) return;
    uint8_t out[3] = {bg.c[0], bg.c[1], bg.c[2]};
    const unsigned long long key = keys[pix];
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
                // (a, b, c): the triangle as mesh_raster.hip's raster_setup orders it, vertices 1 and 2 exchanged when the area
                // is negative; e_k, q_k and the weights are that triangle's, as resolve forms them
                const bool flip = As < 0;
                const int64_t px = 256ll * (pix % W), py = 256ll * (pix / W);
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
                const double w1 = flip ? wc : wb, w2 = flip ? wb : wc;   // back in the face's own order
                const double dm = (double)(n - 3);
                const double xr = w1 * dm, yr = w2 * dm;
                const double x = xr > 0.0 ? (xr < dm ? xr : dm) : 0.0;
                const double ym = dm - x;
                const double y = yr > 0.0 ? (yr < ym ? yr : ym) : 0.0;
                const double fx = floor(x), fy = floor(y);
                const double ax = x - fx, ay = y - fy;
                const int i0 = (int)fx, j0 = (int)fy;
                const int i1 = i0 + 1 < n ? i0 + 1 : n - 1, j1 = j0 + 1 < n ? j0 + 1 : n - 1;      // (0 <= i0, j0 <= n - 3)
                const double w00 = (1.0 - ax) * (1.0 - ay), w10 = ax * (1.0 - ay), w01 = (1.0 - ax) * ay, w11 = ax * ay;
                int x00, y00, x10, y10, x01, y01, x11, y11;
                atlas_of(t, i0, j0, n, C, x00, y00);
                atlas_of(t, i1, j0, n, C, x10, y10);
                atlas_of(t, i0, j1, n, C, x01, y01);
                atlas_of(t, i1, j1, n, C, x11, y11);
                const uint8_t *c00 = atlas + ((int64_t)y00 * aW + x00) * 3, *c10 = atlas + ((int64_t)y10 * aW + x10) * 3;
                const uint8_t *c01 = atlas + ((int64_t)y01 * aW + x01) * 3, *c11 = atlas + ((int64_t)y11 * aW + x11) * 3;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const double s = ((w00 * (double)c00[c] + w10 * (double)c10[c]) + w01 * (double)c01[c]) + w11 * (double)c11[c];
                    out[c] = raster_byte(s);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) rgb[pix * 3 + c] = out[c];
}

// The cells of T triangles fit an atlas of C cells per row and H rows of texels.
inline bool tex_layout_ok(int64_t T, int32_t n, int32_t C, int32_t H, int32_t W) {
    if (C < 1 || W != (int64_t)C * n || H < 1 || H > kTexMaxSide || W > kTexMaxSide) return false;
    const int64_t cells = (T + 1) / 2, rows = (cells + C - 1) / C;
    return rows * n <= H;
}

}  // namespace occ

OCC_API int occnerf_mesh_texel_points(const float *verts, int64_t V, const int32_t *faces, int64_t T, int32_t n, float *pts,
                                      int32_t *status, void *stream) {
    using namespace occ;
    OCC_REQUIRE(n >= kTexMinCell && n <= kTexMaxCell, "mesh_texel_points: n=%d outside %d..%d", n, kTexMinCell, kTexMaxCell);
    const int64_t P = (int64_t)n * (n - 1) / 2;
    OCC_REQUIRE(V >= 0 && V < (1ll << 31), "mesh_texel_points: V=%lld outside 0..2^31-1", (long long)V);
    OCC_REQUIRE(T >= 0 && T < (1ll << 31) && T * P < (1ll << 31), "mesh_texel_points: T=%lld with %lld texels each reaches 2^31",
                (long long)T, (long long)P);
    if (T == 0) return 0;
    OCC_REQUIRE(faces && pts && status && (verts || V == 0), "mesh_texel_points: null argument");
    const int64_t N = T * P;
    hipLaunchKernelGGL(mesh_texel_points_kernel, dim3((unsigned)((N + kTexThreads - 1) / kTexThreads)), dim3(kTexThreads), 0,
                       as_stream(stream), verts, V, faces, T, (int)n, (int)P, pts, status);
    return check_launch("mesh_texel_points");
}

OCC_API int occnerf_mesh_texture_fill(const float *rgb, int64_t T, int32_t n, int32_t C, int32_t H, int32_t W, uint8_t *atlas,
                                      void *stream) {
    using namespace occ;
    OCC_REQUIRE(n >= kTexMinCell && n <= kTexMaxCell, "mesh_texture_fill: n=%d outside %d..%d", n, kTexMinCell, kTexMaxCell);
    const int64_t P = (int64_t)n * (n - 1) / 2;
    OCC_REQUIRE(T >= 0 && T < (1ll << 31) && T * P < (1ll << 31), "mesh_texture_fill: T=%lld with %lld texels each reaches 2^31",
                (long long)T, (long long)P);
    OCC_REQUIRE(tex_layout_ok(T, n, C, H, W), "mesh_texture_fill: an atlas of H=%d W=%d with C=%d cells of %d per row does not hold "
                "T=%lld triangles (W = C n, rows of cells * n <= H <= %d)", H, W, C, n, (long long)T, kTexMaxSide);
    if (T == 0) return 0;
    OCC_REQUIRE(rgb && atlas, "mesh_texture_fill: null argument");
    const int64_t N = T * P;
    hipLaunchKernelGGL(mesh_texture_fill_kernel, dim3((unsigned)((N + kTexThreads - 1) / kTexThreads)), dim3(kTexThreads), 0,
                       as_stream(stream), rgb, T, (int)n, (int)P, (int)C, (int)W, atlas);
    return check_launch("mesh_texture_fill");
}

OCC_API int occnerf_mesh_resolve_textured(const uint64_t *keys, const int32_t *faces, int64_t T, int64_t V, const int32_t *xy,
                                          const double *z, int32_t Himg, int32_t Wimg, const uint8_t *atlas, int32_t aH, int32_t aW,
                                          int32_t n, int32_t C, const uint8_t *h_bgcolor, uint8_t *rgb, void *stream) {
    using namespace occ;
    OCC_REQUIRE(h_bgcolor, "mesh_resolve_textured: null argument");
    OCC_REQUIRE(raster_size_ok(Himg, Wimg),
                "mesh_resolve_textured: H=%d W=%d outside 1..16384 or more than 2^28 pixels", Himg, Wimg);
    OCC_REQUIRE(n >= kTexMinCell && n <= kTexMaxCell, "mesh_resolve_textured: n=%d outside %d..%d", n, kTexMinCell, kTexMaxCell);
    OCC_REQUIRE(T >= 0 && T < (1ll << 31), "mesh_resolve_textured: T=%lld outside 0..2^31-1", (long long)T);
    OCC_REQUIRE(V >= 0 && V < (1ll << 31), "mesh_resolve_textured: V=%lld outside 0..2^31-1", (long long)V);
    OCC_REQUIRE(keys && rgb, "mesh_resolve_textured: null argument");
    if (T > 0 && V > 0) {
        OCC_REQUIRE(tex_layout_ok(T, n, C, aH, aW), "mesh_resolve_textured: an atlas of H=%d W=%d with C=%d cells of %d per row does "
                    "not hold T=%lld triangles (W = C n, rows of cells * n <= H <= %d)", aH, aW, C, n, (long long)T, kTexMaxSide);
        OCC_REQUIRE(faces && xy && z && atlas, "mesh_resolve_textured: null argument");
    }
    RasterBg bg;
    for (int c = 0; c < 3; c++) bg.c[c] = h_bgcolor[c];
    const int64_t N = (int64_t)Himg * Wimg;
    const int64_t Tk = (T > 0 && V > 0) ? T : 0;      // no triangle: no key names one (t < 0 fails), the background everywhere
    hipLaunchKernelGGL(mesh_resolve_textured_kernel, dim3((unsigned)((N + kTexThreads - 1) / kTexThreads)), dim3(kTexThreads), 0,
                       as_stream(stream), (const unsigned long long *)keys, faces, Tk, V, xy, z, (int)Himg, (int)Wimg, atlas, (int)aW,
                       (int)n, (int)C, bg, rgb);
    return check_launch("mesh_resolve_textured");
}
