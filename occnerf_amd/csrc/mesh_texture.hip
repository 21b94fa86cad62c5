// The texture of the exported mesh (occnerf_amd/mesh.py bake_texture / export_texture): a per-triangle atlas.
// Triangles 2c and 2c + 1 share the n x n cell c; the even one owns the texels i + j <= n - 2 of the cell, the odd one those of
// the mirrored frame i' = n - 1 - i, j' = n - 1 - j; every triangle owns P = n (n - 1) / 2 texels, numbered by ascending j',
// then ascending i'; texel (i', j') stands for the barycentric numerators (m - i' - j', i', j') over m = n - 3.
//
//   mesh_texel_points       one thread per texel: its canonical point, the colour field's query;
//   mesh_texture_fill       one thread per texel: the queried colour as a byte at its place in the atlas;
//   mesh_resolve_textured   one thread per pixel of mesh_raster's keys: the winner's perspective-correct weights
//                           (mesh_screen.h), then four taps of the atlas (mesh_atlas.h), all of them the winner's own texels.
//   mesh_texture_project    the photographs on the atlas, one frame per call: one thread per triangle for
//                           its weight in this frame, then one thread per texel: seen or not, four taps of the photograph in
//                           integers, its own row of the int64 accumulators;
//   mesh_texture_blend      one thread per texel: the accumulators' rounded mean into the atlas, the seen count into its image.
//
// fp64 on the float32 inputs with + - * / floor rint and comparisons only, one rounding per operator in the order of
// tests/mesh_texture_restatement.py (the tree is built with -ffp-contract=off); the fill's product is the float32 one of
// image.to_8b_image.  No atomics; every output is a pure function of the inputs: the same bytes on every run.  Every index read
// from faces or from a key is checked before it is used as an address, and every atlas address lies inside the C x R cells the
// entry has checked against the atlas' size.  The camera and the vertex rule's three limits, dot3, the winner of a pixel, the
// background and the byte store are mesh_screen.h's; the texel walk, the sampler and the entries' refusals on n, T P and the
// atlas' shape are mesh_atlas.h's.
#include "common.h"
#include "mesh_atlas.h"
#include "mesh_screen.h"

namespace occ {

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
    int i, j, x, y;
    texel_walk(g, n, P, C, i, j, x, y);
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
    ScreenWinner win;
    if (screen_winner(keys[pix], faces, T, V, xy, z, pix, W, win)) {
        const AtlasTaps taps = atlas_taps(atlas, aW, win.t, win.w1, win.w2, n, C);
#pragma unroll
        for (int c = 0; c < 3; c++) out[c] = raster_byte(taps.blend(c));
    }
#pragma unroll
    for (int c = 0; c < 3; c++) rgb[pix * 3 + c] = out[c];
}

// ---------------------------------------------------------------- the photographs on the atlas
// The vertex rule of mesh_screen.h's screen_vertex, stated again without the coordinates it hands back: calling screen_vertex
// here compiled the weights to other code, which ran outside the parent's range in two of six traced runs (DESIGN.md section
// 7o).  The camera and the three limits are the header's.
__device__ __forceinline__ int photo_vertex(const ScreenCamera &cam, const float *__restrict__ p, double c[3]) {
    const double p0 = (double)p[0], p1 = (double)p[1], p2 = (double)p[2];
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = ((cam.R[k * 3] * p0 + cam.R[k * 3 + 1] * p1) + cam.R[k * 3 + 2] * p2) + cam.t[k];
    const double a = 256.0 * (cam.fx * (c[0] / c[2]) + cam.cx);
    const double b = 256.0 * (cam.fy * (c[1] / c[2]) + cam.cy);
    if (!(c[2] >= kScreenNear)) return 1;
    if (!(fabs(a) <= kScreenGuard && fabs(b) <= kScreenGuard && c[2] <= kScreenFar)) return 2;
    return 0;
}

// The weight of a triangle in one frame: 1 .. 256, 0 (unusable: flagged, degenerate, grazing) or -1 (it faces away).
__global__ __launch_bounds__(kTexThreads) void mesh_photo_weight_kernel(const float *__restrict__ verts,
                                                                        const uint8_t *__restrict__ pflag, int64_t V,
                                                                        const int32_t *__restrict__ faces, int64_t T, ScreenCamera cam,
                                                                        int32_t *__restrict__ tw, int32_t *__restrict__ status) {
    const int64_t t = (int64_t)blockIdx.x * kTexThreads + threadIdx.x;
    if (t >= T) return;
    const int32_t v0 = faces[t * 3], v1 = faces[t * 3 + 1], v2 = faces[t * 3 + 2];
    if (v0 < 0 || v0 >= V || v1 < 0 || v1 >= V || v2 < 0 || v2 >= V) {
        tw[t] = 0;
        status[0] = 1;                          // every thread that gets here stores the same value
        return;
    }
    double c0[3], c1[3], c2[3];
    int flag = pflag[v0] | pflag[v1] | pflag[v2];
    flag |= photo_vertex(cam, verts + (int64_t)v0 * 3, c0);
    flag |= photo_vertex(cam, verts + (int64_t)v1 * 3, c1);
    flag |= photo_vertex(cam, verts + (int64_t)v2 * 3, c2);
    int w = 0;
    if (flag == 0) {
        double e1[3], e2[3], g[3], N[3];
#pragma unroll
        for (int k = 0; k < 3; k++) e1[k] = c1[k] - c0[k], e2[k] = c2[k] - c0[k], g[k] = (c0[k] + c1[k]) + c2[k];
        N[0] = e1[1] * e2[2] - e1[2] * e2[1];
        N[1] = e1[2] * e2[0] - e1[0] * e2[2];
        N[2] = e1[0] * e2[1] - e1[1] * e2[0];
        const double d = dot3(N, g), NN = dot3(N, N), gg = dot3(g, g);
        const double q = NN * gg;
        const double r = 256.0 * ((d * d) / q);
        if (q > 0.0 && q <= 1.7976931348623157e308 && r >= 0.0 && r <= 1.7976931348623157e308) {        // (a NaN fails)
            if (d > 0.0) w = -1;                // the outward normal points along the line of sight: the far side
            else {
                const double rr = rint(r);
                w = rr < 256.0 ? (int)rr : 256;
            }
        }
    }
    tw[t] = w;
}

__global__ __launch_bounds__(kTexThreads) void mesh_texture_project_kernel(
    const int32_t *__restrict__ xy, const double *__restrict__ z, const uint8_t *__restrict__ vflag, int64_t N, int P,
    const int32_t *__restrict__ tw, const unsigned long long *__restrict__ keys, const uint8_t *__restrict__ photo,
    const uint8_t *__restrict__ inside, int H, int W, double bias, long long *__restrict__ acc, int32_t *__restrict__ seen) {
    const int64_t g = (int64_t)blockIdx.x * kTexThreads + threadIdx.x;
    if (g >= N) return;
    const int w = tw[g / P];
    if (w <= 0 || vflag[g] != 0) return;
    const int2 s = *reinterpret_cast<const int2 *>(xy + g * 2);
    const int j0 = s.x >> 8, i0 = s.y >> 8;
    if (j0 < 0 || i0 < 0 || j0 + 1 >= W || i0 + 1 >= H) return;           // no tap address before this test
    const int64_t a00 = (int64_t)i0 * W + j0, a10 = a00 + W;
    if ((inside[a00] == 0) | (inside[a00 + 1] == 0) | (inside[a10] == 0) | (inside[a10 + 1] == 0)) return;
    const double zq = z[g];
    const int64_t tap[4] = {a00, a00 + 1, a10, a10 + 1};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned long long key = keys[tap[k]];
        if (key == kRasterEmpty) return;
        if (!(zq <= (double)__uint_as_float((unsigned)(key >> 32)) + bias)) return;
    }
    const int fx = s.x & 255, fy = s.y & 255;
    const int w00 = (256 - fx) * (256 - fy), w01 = fx * (256 - fy), w10 = (256 - fx) * fy, w11 = fx * fy;
    long long a[4];
    {
        const longlong2 lo = *reinterpret_cast<const longlong2 *>(acc + g * 4), hi = *reinterpret_cast<const longlong2 *>(acc + g * 4 + 2);
        a[0] = lo.x, a[1] = lo.y, a[2] = hi.x, a[3] = hi.y;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int sum = w00 * (int)photo[tap[0] * 3 + c] + w01 * (int)photo[tap[1] * 3 + c] + w10 * (int)photo[tap[2] * 3 + c] +
                        w11 * (int)photo[tap[3] * 3 + c];                 // <= 65536 * 255
        a[c] += (long long)w * (long long)sum;
    }
    a[3] += (long long)w;
    *reinterpret_cast<longlong2 *>(acc + g * 4) = make_longlong2(a[0], a[1]);
    *reinterpret_cast<longlong2 *>(acc + g * 4 + 2) = make_longlong2(a[2], a[3]);
    seen[g] += 1;
}

__global__ __launch_bounds__(kTexThreads) void mesh_texture_blend_kernel(const long long *__restrict__ acc,
                                                                         const int32_t *__restrict__ seen, int64_t T, int n, int P,
                                                                         int C, int W, int min_seen, uint8_t *__restrict__ atlas,
                                                                         uint8_t *__restrict__ seen_img) {
    const int64_t g = (int64_t)blockIdx.x * kTexThreads + threadIdx.x;
    if (g >= T * P) return;
    int i, j, x, y;
    texel_walk(g, n, P, C, i, j, x, y);
    const int64_t at = (int64_t)y * W + x;
    const int32_t s = seen[g];
    seen_img[at] = (uint8_t)(s < 0 ? 0 : (s < 255 ? s : 255));
    const longlong2 lo = *reinterpret_cast<const longlong2 *>(acc + g * 4), hi = *reinterpret_cast<const longlong2 *>(acc + g * 4 + 2);
    const long long a3 = hi.y;
    if (s < min_seen || a3 <= 0) return;                                   // the field's byte stays
    const long long a[3] = {lo.x, lo.y, hi.x};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const long long v = (a[c] + 32768ll * a3) / (65536ll * a3);
        atlas[at * 3 + c] = (uint8_t)(v > 0 ? (v < 255 ? v : 255) : 0);
    }
}

}  // namespace occ

OCC_API int occnerf_mesh_texel_points(const float *verts, int64_t V, const int32_t *faces, int64_t T, int32_t n, float *pts,
                                      int32_t *status, void *stream) {
    using namespace occ;
    if (!tex_cell_ok("mesh_texel_points", n)) return 1;
    OCC_REQUIRE(V >= 0 && V < (1ll << 31), "mesh_texel_points: V=%lld outside 0..2^31-1", (long long)V);
    int64_t P;
    if (!tex_count_ok("mesh_texel_points", T, n, P)) return 1;
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
    if (!tex_cell_ok("mesh_texture_fill", n)) return 1;
    int64_t P;
    if (!tex_count_ok("mesh_texture_fill", T, n, P) || !tex_atlas_ok("mesh_texture_fill", T, n, C, H, W)) return 1;
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
    if (!tex_cell_ok("mesh_resolve_textured", n)) return 1;
    OCC_REQUIRE(T >= 0 && T < (1ll << 31), "mesh_resolve_textured: T=%lld outside 0..2^31-1", (long long)T);
    OCC_REQUIRE(V >= 0 && V < (1ll << 31), "mesh_resolve_textured: V=%lld outside 0..2^31-1", (long long)V);
    OCC_REQUIRE(keys && rgb, "mesh_resolve_textured: null argument");
    if (T > 0 && V > 0) {
        if (!tex_atlas_ok("mesh_resolve_textured", T, n, C, aH, aW)) return 1;
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

OCC_API int occnerf_mesh_texture_project(const int32_t *xy, const double *z, const uint8_t *vflag, const float *verts,
                                         const uint8_t *pflag, int64_t V, const int32_t *faces, int64_t T, int32_t n,
                                         const double *h_K, const double *h_E, const uint64_t *keys, const uint8_t *photo,
                                         const uint8_t *inside, int32_t H, int32_t W, double bias, int64_t *acc, int32_t *seen,
                                         int32_t *tri_w, int32_t *status, void *stream) {
    using namespace occ;
    OCC_REQUIRE(h_K && h_E, "mesh_texture_project: null argument");
    OCC_REQUIRE(h_K[1] == 0.0, "mesh_texture_project: skew K[0,1] = %g is not built", h_K[1]);
    if (!tex_cell_ok("mesh_texture_project", n)) return 1;
    OCC_REQUIRE(H >= 1 && H <= kTexMaxSide && W >= 1 && W <= kTexMaxSide, "mesh_texture_project: H=%d W=%d outside 1..%d", H, W,
                kTexMaxSide);
    OCC_REQUIRE(bias >= 0.0, "mesh_texture_project: bias=%g is negative or not a number", bias);
    OCC_REQUIRE(V >= 0 && V < (1ll << 31), "mesh_texture_project: V=%lld outside 0..2^31-1", (long long)V);
    int64_t P;
    if (!tex_count_ok("mesh_texture_project", T, n, P)) return 1;
    if (T == 0) return 0;
    OCC_REQUIRE(xy && z && vflag && faces && keys && photo && inside && acc && seen && tri_w && status && ((verts && pflag) || V == 0),
                "mesh_texture_project: null argument");
    hipLaunchKernelGGL(mesh_photo_weight_kernel, dim3((unsigned)((T + kTexThreads - 1) / kTexThreads)), dim3(kTexThreads), 0,
                       as_stream(stream), verts, pflag, V, faces, T, screen_camera(h_K, h_E), tri_w, status);
    if (int rc = check_launch("mesh_texture_project (weights)")) return rc;
    const int64_t N = T * P;
    hipLaunchKernelGGL(mesh_texture_project_kernel, dim3((unsigned)((N + kTexThreads - 1) / kTexThreads)), dim3(kTexThreads), 0,
                       as_stream(stream), xy, z, vflag, N, (int)P, tri_w, (const unsigned long long *)keys, photo, inside, (int)H,
                       (int)W, bias, (long long *)acc, seen);
    return check_launch("mesh_texture_project");
}

OCC_API int occnerf_mesh_texture_blend(const int64_t *acc, const int32_t *seen, int64_t T, int32_t n, int32_t C, int32_t H,
                                       int32_t W, int32_t min_seen, uint8_t *atlas, uint8_t *seen_img, void *stream) {
    using namespace occ;
    if (!tex_cell_ok("mesh_texture_blend", n)) return 1;
    OCC_REQUIRE(min_seen >= 1, "mesh_texture_blend: min_seen=%d is not a whole number >= 1", min_seen);
    int64_t P;
    if (!tex_count_ok("mesh_texture_blend", T, n, P) || !tex_atlas_ok("mesh_texture_blend", T, n, C, H, W)) return 1;
    if (T == 0) return 0;
    OCC_REQUIRE(acc && seen && atlas && seen_img, "mesh_texture_blend: null argument");
    const int64_t N = T * P;
    hipLaunchKernelGGL(mesh_texture_blend_kernel, dim3((unsigned)((N + kTexThreads - 1) / kTexThreads)), dim3(kTexThreads), 0,
                       as_stream(stream), (const long long *)acc, seen, T, (int)n, (int)P, (int)C, (int)W, (int)min_seen, atlas,
                       seen_img);
    return check_launch("mesh_texture_blend");
}
