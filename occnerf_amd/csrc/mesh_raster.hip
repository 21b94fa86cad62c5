// A triangle mesh seen through a frame's camera (occnerf_amd/mesh_view.py rasterize): coverage, the
// nearest triangle per pixel, its depth and its interpolated vertex colour.  Three entries:
//
//   project   one thread per vertex: the camera transform and the pinhole projection in fp64, snapped to 1/256 pixel;
//   raster    one thread per triangle walks the samples of its clipped bounding box -- the typical load is hundreds of thousands
//             of triangles smaller than a pixel, most threads find no sample or one -- and merges every covered sample into
//             the pixel's 64-bit key (float32 depth bits << 32 | triangle index) with an unsigned atomic minimum.  A triangle
//             whose box holds more than kRasterWide samples is appended to a list instead and drawn by a second launch, one
//             wave per listed triangle with the lanes over the box's samples.  The list's order varies from run to run; the
//             image does not depend on it;
//   resolve   one thread per pixel: the winner's colour from its key.
//
// The minimum is commutative and idempotent, so the image is the same bytes on every run, whatever order the triangles
// arrive in and from whichever XCD (relaxed, agent scope; resolve is a later launch on the same stream).  A sample first looks
// at the pixel's key with a relaxed load and skips the atomic when it cannot win: keys only ever decrease, so a stale value
// only costs an atomic that was not needed.  The counts are integer sums, one atomic add per wave and counter.
//
// Coverage is int64 arithmetic on the fixed-point coordinates; the fp64 steps use + * / rint and comparisons only, one rounding
// per operator in the order of tests/mesh_raster_restatement.py (the tree is built with -ffp-contract=off): the outputs are that
// file's, bit for bit.  Every index read from faces or from a key is checked before it is used as an address.  The camera with
// its vertex rule and three limits, the empty key, the image-size test, the background and the byte store are mesh_screen.h's,
// shared with mesh_texture.hip and mesh_normal.hip.
#include "common.h"
#include "mesh_screen.h"

namespace occ {

constexpr int kRasterThreads = 256;
constexpr int kRasterWide = 64;                   // samples in the clipped box above which a triangle goes to the wide pass
constexpr int kRasterWideBlocks = 1024;           // of kRasterThreads: 4096 waves stride over the list
constexpr int kRasterMaxSide = 16384;
constexpr int64_t kRasterMaxPixels = 1ll << 28;
enum RasterCount : int { kCntIndex = 0, kCntNear, kCntGuard, kCntArea, kCntOffscreen, kCntWide, kCntCovered, kCntTotal };

__global__ __launch_bounds__(kRasterThreads) void mesh_project_kernel(const float *__restrict__ pos, int64_t V, ScreenCamera cam,
                                                                      int32_t *__restrict__ xy, double *__restrict__ z,
                                                                      uint8_t *__restrict__ vflag) {
    const int64_t i = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
    if (i >= V) return;
    double c[3], a, b;
    const int flag = screen_vertex(cam, pos + i * 3, c, a, b);
    xy[i * 2] = flag ? 0 : (int32_t)rint(a);
    xy[i * 2 + 1] = flag ? 0 : (int32_t)rint(b);
    z[i] = flag ? 0.0 : c[2];
    vflag[i] = (uint8_t)flag;
}

struct RasterTri {
    int32_t v[3];             // vertex indices, 1 and 2 exchanged when the area was negative
    int64_t X[3], Y[3];
    int64_t A;                // > 0
};

// 0: kept; else 1 + the RasterCount of the reason it is dropped for.
__device__ __forceinline__ int raster_setup(const int32_t *__restrict__ faces, int64_t t, int64_t V, const int32_t *__restrict__ xy,
                                            const uint8_t *__restrict__ vflag, RasterTri &tr) {
    int32_t v[3];
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = faces[t * 3 + k];
    if (v[0] < 0 || v[0] >= V || v[1] < 0 || v[1] >= V || v[2] < 0 || v[2] >= V) return 1 + kCntIndex;
    const int f0 = vflag[v[0]], f1 = vflag[v[1]], f2 = vflag[v[2]];
    if (f0 == 1 || f1 == 1 || f2 == 1) return 1 + kCntNear;
    if (f0 == 2 || f1 == 2 || f2 == 2) return 1 + kCntGuard;
    int64_t X[3], Y[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int2 p = *reinterpret_cast<const int2 *>(xy + (int64_t)v[k] * 2);
        X[k] = p.x, Y[k] = p.y;
    }
    const int64_t A = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]);
    if (A == 0) return 1 + kCntArea;
    const bool flip = A < 0;
    tr.v[0] = v[0], tr.X[0] = X[0], tr.Y[0] = Y[0];
    tr.v[1] = flip ? v[2] : v[1], tr.X[1] = flip ? X[2] : X[1], tr.Y[1] = flip ? Y[2] : Y[1];
    tr.v[2] = flip ? v[1] : v[2], tr.X[2] = flip ? X[1] : X[2], tr.Y[2] = flip ? Y[1] : Y[2];
    tr.A = flip ? -A : A;
    return 0;
}

__device__ __forceinline__ int64_t lo64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t hi64(int64_t a, int64_t b) { return a > b ? a : b; }

// The columns [j0, j1] and rows [i0, i1] whose samples lie in the triangle's bounding box, clipped to the image; false when
// the box misses the image altogether.
__device__ __forceinline__ bool raster_box(const RasterTri &tr, int H, int W, int &j0, int &j1, int &i0, int &i1) {
    const int64_t x0 = lo64(tr.X[0], lo64(tr.X[1], tr.X[2])), x1 = hi64(tr.X[0], hi64(tr.X[1], tr.X[2]));
    const int64_t y0 = lo64(tr.Y[0], lo64(tr.Y[1], tr.Y[2])), y1 = hi64(tr.Y[0], hi64(tr.Y[1], tr.Y[2]));
    if (x1 < 0 || x0 > 256ll * (W - 1) || y1 < 0 || y0 > 256ll * (H - 1)) return false;
    j0 = (int)hi64(0, (x0 + 255) >> 8), j1 = (int)lo64(W - 1, x1 >> 8);
    i0 = (int)hi64(0, (y0 + 255) >> 8), i1 = (int)lo64(H - 1, y1 >> 8);
    return true;
}

// The three edge functions at the sample of pixel (i, j); true when the sample is covered (top-left rule).
__device__ __forceinline__ bool raster_edges(const RasterTri &tr, int i, int j, int64_t (&e)[3]) {
    const int64_t px = 256ll * j, py = 256ll * i;
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        const int64_t dx = tr.X[b] - tr.X[a], dy = tr.Y[b] - tr.Y[a];
        e[k] = dx * (py - tr.Y[a]) - dy * (px - tr.X[a]);
        in = in && (e[k] > 0 || (e[k] == 0 && (dy < 0 || (dy == 0 && dx > 0))));
    }
    return in;
}

// q_k = (e_k / A) / z_k and their sum, the inverse depth.
__device__ __forceinline__ double raster_inverse_depth(const int64_t (&e)[3], int64_t A, const double (&z)[3], double (&q)[3]) {
    const double a = (double)A;
#pragma unroll
    for (int k = 0; k < 3; k++) q[k] = ((double)e[k] / a) / z[k];
    return (q[0] + q[1]) + q[2];
}

__device__ __forceinline__ void raster_sample(const RasterTri &tr, const double (&z)[3], int64_t t, int i, int j, int W,
                                              unsigned long long *__restrict__ keys) {
    int64_t e[3];
    if (!raster_edges(tr, i, j, e)) return;
    double q[3];
    const float depth = (float)(1.0 / raster_inverse_depth(e, tr.A, z, q));
    const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)(uint32_t)t;
    unsigned long long *slot = keys + (int64_t)i * W + j;
    if (key < __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        __hip_atomic_fetch_min(slot, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void raster_count(bool mine, int32_t *counter) {
    const unsigned long long m = __ballot(mine);
    if (m != 0 && (threadIdx.x & (kWave - 1)) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(counter, __popcll(m));
}

__global__ __launch_bounds__(kRasterThreads) void mesh_raster_kernel(
    const int32_t *__restrict__ faces, int64_t T, int64_t V, const int32_t *__restrict__ xy, const uint8_t *__restrict__ vflag,
    const double *__restrict__ z, int H, int W, unsigned long long *__restrict__ keys, int32_t *__restrict__ wide_list,
    int32_t *__restrict__ counts) {
    const int64_t t = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
    RasterTri tr;
    int j0 = 0, j1 = -1, i0 = 0, i1 = -1;
    int reason = -1;                                          // a thread past T
    if (t < T) {
        reason = raster_setup(faces, t, V, xy, vflag, tr);
        if (reason == 0 && !raster_box(tr, H, W, j0, j1, i0, i1)) reason = 1 + kCntOffscreen;
    }
#pragma unroll
    for (int r = 0; r <= kCntOffscreen; r++) raster_count(reason == 1 + r, counts + r);
    if (reason != 0 || j1 < j0 || i1 < i0) return;
    const int64_t n = (int64_t)(j1 - j0 + 1) * (i1 - i0 + 1);
    if (n > kRasterWide) {
        const int32_t slot = atomicAdd(counts + kCntWide, 1);         // every triangle is listed at most once: T entries suffice
        if (slot >= 0 && slot < T) wide_list[slot] = (int32_t)t;      // (a count the caller did not zero must not become an address)
        return;
    }
    const double zz[3] = {z[tr.v[0]], z[tr.v[1]], z[tr.v[2]]};
    for (int i = i0; i <= i1; i++)
        for (int j = j0; j <= j1; j++) raster_sample(tr, zz, t, i, j, W, keys);
}

// One wave per listed triangle, the lanes over the samples of its box.
__global__ __launch_bounds__(kRasterThreads) void mesh_raster_wide_kernel(
    const int32_t *__restrict__ faces, int64_t T, int64_t V, const int32_t *__restrict__ xy, const uint8_t *__restrict__ vflag,
    const double *__restrict__ z, int H, int W, unsigned long long *__restrict__ keys, const int32_t *__restrict__ wide_list,
    const int32_t *__restrict__ counts) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t n_list = lo64(counts[kCntWide], T);
    const int64_t waves = (int64_t)gridDim.x * (kRasterThreads / kWave);
    for (int64_t w = (int64_t)blockIdx.x * (kRasterThreads / kWave) + threadIdx.x / kWave; w < n_list; w += waves) {
        const int64_t t = wide_list[w];
        if (t < 0 || t >= T) continue;
        RasterTri tr;
        int j0, j1, i0, i1;
        if (raster_setup(faces, t, V, xy, vflag, tr) != 0 || !raster_box(tr, H, W, j0, j1, i0, i1)) continue;
        const double zz[3] = {z[tr.v[0]], z[tr.v[1]], z[tr.v[2]]};
        const int bw = j1 - j0 + 1;
        const int64_t n = (int64_t)bw * (i1 - i0 + 1);
        for (int64_t s = lane; s < n; s += kWave) raster_sample(tr, zz, t, i0 + (int)(s / bw), j0 + (int)(s % bw), W, keys);
    }
}

__global__ __launch_bounds__(kRasterThreads) void mesh_resolve_kernel(
    const unsigned long long *__restrict__ keys, const int32_t *__restrict__ faces, int64_t T, int64_t V,
    const int32_t *__restrict__ xy, const uint8_t *__restrict__ vflag, const double *__restrict__ z,
    const uint8_t *__restrict__ colors, RasterBg bg, int H, int W, uint8_t *__restrict__ cover, int32_t *__restrict__ tri,
    float *__restrict__ depth, uint8_t *__restrict__ rgb, int32_t *__restrict__ counts) {
    const int64_t pix = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
    const bool live = pix < (int64_t)H * W;
    bool hit = false;
    if (live) {
        const unsigned long long key = keys[pix];
        const int64_t t = (int64_t)(key & 0xFFFFFFFFull);
        RasterTri tr;
        hit = key != kRasterEmpty && t < T && raster_setup(faces, t, V, xy, vflag, tr) == 0;
        uint8_t out[3] = {bg.c[0], bg.c[1], bg.c[2]};
        if (hit) {
            int64_t e[3];
            raster_edges(tr, (int)(pix / W), (int)(pix % W), e);
            const double zz[3] = {z[tr.v[0]], z[tr.v[1]], z[tr.v[2]]};
            double q[3];
            const double iz = raster_inverse_depth(e, tr.A, zz, q);
            const double w0 = q[0] / iz, w1 = q[1] / iz, w2 = q[2] / iz;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double s = (w0 * (double)colors[(int64_t)tr.v[0] * 3 + c] + w1 * (double)colors[(int64_t)tr.v[1] * 3 + c]) +
                                 w2 * (double)colors[(int64_t)tr.v[2] * 3 + c];
                out[c] = raster_byte(s);      // (a NaN cannot arise: iz > 0)
            }
        }
        cover[pix] = hit ? 1 : 0;
        tri[pix] = hit ? (int32_t)t : -1;
        depth[pix] = hit ? __uint_as_float((uint32_t)(key >> 32)) : __uint_as_float(0x7F800000u);
#pragma unroll
        for (int c = 0; c < 3; c++) rgb[pix * 3 + c] = out[c];
    }
    raster_count(hit, counts + kCntCovered);
}

bool raster_size_ok(int32_t H, int32_t W) {
    return H >= 1 && W >= 1 && H <= kRasterMaxSide && W <= kRasterMaxSide && (int64_t)H * W <= kRasterMaxPixels;
}

}  // namespace occ

OCC_API int occnerf_mesh_project(const float *pos, int64_t V, const double *h_K, const double *h_E, int32_t *xy, double *z,
                                 uint8_t *vflag, void *stream) {
    using namespace occ;
    OCC_REQUIRE(h_K && h_E, "mesh_project: null argument");
    OCC_REQUIRE(h_K[1] == 0.0, "mesh_project: skew K[0,1] = %g is not built", h_K[1]);
    OCC_REQUIRE(V >= 0 && V < (1ll << 31), "mesh_project: V=%lld outside 0..2^31-1", (long long)V);
    if (V == 0) return 0;
    OCC_REQUIRE(pos && xy && z && vflag, "mesh_project: null pos / output with V=%lld", (long long)V);
    hipLaunchKernelGGL(mesh_project_kernel, dim3((unsigned)((V + kRasterThreads - 1) / kRasterThreads)), dim3(kRasterThreads), 0,
                       as_stream(stream), pos, V, screen_camera(h_K, h_E), xy, z, vflag);
    return check_launch("mesh_project");
}

OCC_API int occnerf_mesh_raster(const int32_t *faces, int64_t T, int64_t V, const int32_t *xy, const double *z,
                                const uint8_t *vflag, int32_t H, int32_t W, uint64_t *keys, int32_t *wide_list, int32_t *counts,
                                void *stream) {
    using namespace occ;
    OCC_REQUIRE(raster_size_ok(H, W), "mesh_raster: H=%d W=%d outside 1..%d or more than 2^28 pixels", H, W, kRasterMaxSide);
    OCC_REQUIRE(T >= 0 && T < (1ll << 31), "mesh_raster: T=%lld outside 0..2^31-1", (long long)T);
    OCC_REQUIRE(V >= 0 && V < (1ll << 31), "mesh_raster: V=%lld outside 0..2^31-1", (long long)V);
    if (T == 0 || V == 0) return 0;
    OCC_REQUIRE(faces && xy && z && vflag && keys && wide_list && counts, "mesh_raster: null argument");
    hipLaunchKernelGGL(mesh_raster_kernel, dim3((unsigned)((T + kRasterThreads - 1) / kRasterThreads)), dim3(kRasterThreads), 0,
                       as_stream(stream), faces, T, V, xy, vflag, z, (int)H, (int)W, (unsigned long long *)keys, wide_list, counts);
    int rc = check_launch("mesh_raster");
    if (rc) return rc;
    hipLaunchKernelGGL(mesh_raster_wide_kernel, dim3(kRasterWideBlocks), dim3(kRasterThreads), 0, as_stream(stream), faces, T, V,
                       xy, vflag, z, (int)H, (int)W, (unsigned long long *)keys, (const int32_t *)wide_list,
                       (const int32_t *)counts);
    return check_launch("mesh_raster (wide pass)");
}

OCC_API int occnerf_mesh_resolve(const uint64_t *keys, const int32_t *faces, int64_t T, int64_t V, const int32_t *xy,
                                 const double *z, const uint8_t *vflag, const uint8_t *colors, const uint8_t *h_bgcolor,
                                 int32_t H, int32_t W, uint8_t *cover, int32_t *tri, float *depth, uint8_t *rgb, int32_t *counts,
                                 void *stream) {
    using namespace occ;
    OCC_REQUIRE(h_bgcolor, "mesh_resolve: null argument");
    OCC_REQUIRE(raster_size_ok(H, W), "mesh_resolve: H=%d W=%d outside 1..%d or more than 2^28 pixels", H, W, kRasterMaxSide);
    OCC_REQUIRE(T >= 0 && T < (1ll << 31), "mesh_resolve: T=%lld outside 0..2^31-1", (long long)T);
    OCC_REQUIRE(V >= 0 && V < (1ll << 31), "mesh_resolve: V=%lld outside 0..2^31-1", (long long)V);
    if (T == 0 || V == 0) return 0;
    OCC_REQUIRE(keys && faces && xy && z && vflag && colors && cover && tri && depth && rgb && counts,
                "mesh_resolve: null argument");
    RasterBg bg;
    for (int c = 0; c < 3; c++) bg.c[c] = h_bgcolor[c];
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(mesh_resolve_kernel, dim3((unsigned)((n + kRasterThreads - 1) / kRasterThreads)), dim3(kRasterThreads), 0,
                       as_stream(stream), (const unsigned long long *)keys, faces, T, V, xy, vflag, z, colors, bg, (int)H, (int)W,
                       cover, tri, depth, rgb, counts);
    return check_launch("mesh_resolve");
}
