// The tangent-space normal map of the exported mesh (occnerf_amd/mesh.py bake_normal_map / export_normal_map, DESIGN.md section
// 7q): every texel of the coarse mesh's per-triangle atlas (mesh_atlas.h) is projected along the
// interpolated vertex normal onto the iso-surface of a fine density grid, and the field's normal there is stored in the tangent
// frame the glTF carries.
//
//   mesh_normal_bake    one thread per texel: the search direction, 2 S + 1 trilinear samples along it, the nearest crossing of
//                       the level, six samples for the central difference there, the normal in the frame [T B n] by the cofactor
//                       formula, three bytes at the texel's place in the atlas; the offset, the flags and the object-space normal
//                       per texel beside it;
//   mesh_resolve_lit    one thread per pixel of mesh_raster's keys: the winner's perspective-correct weights (mesh_screen.h),
//                       the interpolated corner normal and tangent, the normal atlas through section 7o's sampler (mesh_atlas.h,
//                       the blend kept unrounded), and two grey panels by section 7k's headlight rule: the geometry's normal
//                       alone and the mapped one.
//
// fp64 on the float32 inputs with + - * / sqrt floor rint and comparisons only, one rounding per operator in the order of
// tests/mesh_normal_restatement.py (the tree is built with -ffp-contract=off).  No atomics, no LDS; every output is a pure function
// of the inputs: the same bytes on every run.  Every index read from faces or from a key is checked before it is used as an
// address; every grid address is formed from a coordinate clamped to [0, n_a - 1] and a cell clamped to [0, n_a - 2] (a NaN
// coordinate clamps to 0), so it lies inside the grid the entry has checked to have two points per axis; every atlas address lies
// inside the C x R cells the entry has checked against the atlas' size.
//
// The eight taps of a sample are four pairs of neighbouring floats (x fastest); neighbouring texels of a triangle are a fraction
// of a fine voxel apart and walk along nearly parallel lines, so a wavefront's taps of one step fall into a few cache lines: the
// loads are plain cached global loads, and nothing is staged.
#include "common.h"
#include "mesh_atlas.h"
#include "mesh_screen.h"

namespace occ {

constexpr int kNormalMaxSteps = 64;
constexpr double kNormalMinDet = 9.5367431640625e-07;      // 2^-20
constexpr double kFiniteMax = 1.7976931348623157e308;

enum : int { kNormalNoCrossing = 1, kNormalNoGradient = 2, kNormalFlat = 4, kNormalFaceDirection = 8 };

struct NormalGrid {
    int nx, ny, nz;
    double lo[3], h;
    double level;              // the float32 level as a double
    double delta;              // h / 2
    int S;
};

__device__ __forceinline__ bool usable(double l2) { return l2 > 0.0 && l2 <= kFiniteMax; }          // (a NaN fails)
__device__ __forceinline__ bool finite64(double x) { return fabs(x) <= kFiniteMax; }                // (a NaN fails)
__device__ __forceinline__ void cross3(const double a[3], const double b[3], double c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
// v / sqrt(v.v) -> true; v stays and false comes back when v.v is zero or not finite.
__device__ __forceinline__ bool normalise3(double v[3]) {
    const double l2 = dot3(v, v);
    if (!usable(l2)) return false;
    const double l = sqrt(l2);
    v[0] = v[0] / l, v[1] = v[1] / l, v[2] = v[2] / l;
    return true;
}
__device__ __forceinline__ float canonical(double x) { return x == x ? (float)x : __uint_as_float(0x7FC00000u); }

// One axis of the trilinear sample: the cell and the fraction of the clamped grid coordinate.
__device__ __forceinline__ void grid_axis(double q, double lo, double h, int n, int &cell, double &f) {
    const double g = (q - lo) / h, top = (double)(n - 1);
    const double c = g > 0.0 ? (g < top ? g : top) : 0.0;          // (a NaN fails the first comparison: 0)
    const int fl = (int)floor(c);
    cell = fl < n - 2 ? fl : n - 2;
    f = c - (double)cell;
}

__device__ __forceinline__ double trilinear(const float *__restrict__ field, const NormalGrid &G, double qx, double qy, double qz) {
    int ix, iy, iz;
    double fx, fy, fz;
    grid_axis(qx, G.lo[0], G.h, G.nx, ix, fx);
    grid_axis(qy, G.lo[1], G.h, G.ny, iy, fy);
    grid_axis(qz, G.lo[2], G.h, G.nz, iz, fz);
    const float *b = field + ((int64_t)iz * G.ny + iy) * G.nx + ix;
    const int64_t sy = G.nx, sz = (int64_t)G.nx * G.ny;
    const double v000 = (double)b[0], v100 = (double)b[1], v010 = (double)b[sy], v110 = (double)b[sy + 1];
    const double v001 = (double)b[sz], v101 = (double)b[sz + 1], v011 = (double)b[sz + sy], v111 = (double)b[sz + sy + 1];
    const double gx = 1.0 - fx, gy = 1.0 - fy, gz = 1.0 - fz;
    const double c00 = v000 * gx + v100 * fx, c10 = v010 * gx + v110 * fx, c01 = v001 * gx + v101 * fx, c11 = v011 * gx + v111 * fx;
    const double c0 = c00 * gy + c10 * fy, c1 = c01 * gy + c11 * fy;
    return c0 * gz + c1 * fz;
}

__device__ __forceinline__ void load3(const float *__restrict__ p, double v[3]) { v[0] = (double)p[0], v[1] = (double)p[1], v[2] = (double)p[2]; }
// (b0 a + b1 b) + b2 c per coordinate.
__device__ __forceinline__ void blend3(double b0, double b1, double b2, const double a[3], const double b[3], const double c[3],
                                       double out[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) out[k] = (b0 * a[k] + b1 * b[k]) + b2 * c[k];
}

__global__ __launch_bounds__(kTexThreads) void mesh_normal_bake_kernel(
    const float *__restrict__ verts, const float *__restrict__ vnormals, int64_t V, const int32_t *__restrict__ faces, int64_t T,
    const float *__restrict__ tangents, const uint8_t *__restrict__ creased, const float *__restrict__ pts, int n, int P, int C, int W,
    const float *__restrict__ field, NormalGrid G, uint8_t *__restrict__ atlas, float *__restrict__ offset,
    uint8_t *__restrict__ flags, float *__restrict__ normal, int32_t *__restrict__ status) {
    const int64_t g = (int64_t)blockIdx.x * kTexThreads + threadIdx.x;
    if (g >= T * P) return;
    int i, j, ax, ay;
    const int64_t t = texel_walk(g, n, P, C, i, j, ax, ay);
    uint8_t *out = atlas + ((int64_t)ay * W + ax) * 3;
    const int32_t v0 = faces[t * 3], v1 = faces[t * 3 + 1], v2 = faces[t * 3 + 2];
    if (v0 < 0 || v0 >= V || v1 < 0 || v1 >= V || v2 < 0 || v2 >= V) {
        const float nan = __uint_as_float(0x7FC00000u);
        offset[g] = nan, flags[g] = 0;
        normal[g * 3] = nan, normal[g * 3 + 1] = nan, normal[g * 3 + 2] = nan;
        out[0] = 128, out[1] = 128, out[2] = 255;
        status[0] = 1;                          // every thread that gets here stores the same value
        return;
    }
    const double b0 = (double)(n - 3 - i - j), b1 = (double)i, b2 = (double)j;
    int flag = 0;
    // 1. the search direction
    double N0[3], N1[3], N2[3], nh[3];
    load3(vnormals + (int64_t)v0 * 3, N0), load3(vnormals + (int64_t)v1 * 3, N1), load3(vnormals + (int64_t)v2 * 3, N2);
    blend3(b0, b1, b2, N0, N1, N2, nh);
    if (!normalise3(nh)) {
        double p0[3], p1[3], p2[3], e1[3], e2[3];
        load3(verts + (int64_t)v0 * 3, p0), load3(verts + (int64_t)v1 * 3, p1), load3(verts + (int64_t)v2 * 3, p2);
#pragma unroll
        for (int k = 0; k < 3; k++) e1[k] = p1[k] - p0[k], e2[k] = p2[k] - p0[k];
        cross3(e1, e2, nh);
        if (!normalise3(nh)) nh[0] = 0.0, nh[1] = 0.0, nh[2] = 1.0;
        flag |= kNormalFaceDirection;
    }
    // 2. the projection: the crossing of the level nearest the texel, between two samples delta apart
    double p[3];
    load3(pts + g * 3, p);
    double s = 0.0;
    bool found = false;
    double u0 = trilinear(field, G, p[0] + ((double)(-G.S) * G.delta) * nh[0], p[1] + ((double)(-G.S) * G.delta) * nh[1],
                          p[2] + ((double)(-G.S) * G.delta) * nh[2]) - G.level;
    for (int k = -G.S; k < G.S; k++) {
        const double a = (double)(k + 1) * G.delta;
        const double u1 = trilinear(field, G, p[0] + a * nh[0], p[1] + a * nh[1], p[2] + a * nh[2]) - G.level;
        if (finite64(u0) && finite64(u1) && ((u0 > 0.0) != (u1 > 0.0))) {
            const double c = ((double)k + u0 / (u0 - u1)) * G.delta;
            if (!found || fabs(c) < fabs(s) || (fabs(c) == fabs(s) && c > s)) s = c;
            found = true;
        }
        u0 = u1;
    }
    if (!found) flag |= kNormalNoCrossing;
    double q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) q[k] = p[k] + s * nh[k];
    // 3. the field's normal: minus the central difference over one fine voxel to either side
    double gr[3], Nf[3];
    gr[0] = trilinear(field, G, q[0] + G.h, q[1], q[2]) - trilinear(field, G, q[0] - G.h, q[1], q[2]);
    gr[1] = trilinear(field, G, q[0], q[1] + G.h, q[2]) - trilinear(field, G, q[0], q[1] - G.h, q[2]);
    gr[2] = trilinear(field, G, q[0], q[1], q[2] + G.h) - trilinear(field, G, q[0], q[1], q[2] - G.h);
    const double l2 = dot3(gr, gr);
    if (usable(l2)) {
        const double l = sqrt(l2);
        Nf[0] = (-gr[0]) / l, Nf[1] = (-gr[1]) / l, Nf[2] = (-gr[2]) / l;
    } else {
        Nf[0] = nh[0], Nf[1] = nh[1], Nf[2] = nh[2];
        flag |= kNormalNoGradient;
    }
    // 4. the tangent space, as a glTF viewer reconstructs it
    double c[3] = {0.0, 0.0, 1.0};
    bool flat = creased[t] != 0;
    if (!flat) {
        double T0[3], T1[3], T2[3], Th[3], B[3], Bn[3], nT[3], TB[3];
        load3(tangents + (t * 3) * 4, T0), load3(tangents + (t * 3 + 1) * 4, T1), load3(tangents + (t * 3 + 2) * 4, T2);
        blend3(b0, b1, b2, T0, T1, T2, Th);
        flat = !normalise3(Th);
        if (!flat) {
            cross3(nh, Th, B);
            cross3(B, nh, Bn), cross3(nh, Th, nT), cross3(Th, B, TB);
            const double det = dot3(Th, Bn);
            c[0] = dot3(Nf, Bn) / det, c[1] = dot3(Nf, nT) / det, c[2] = dot3(Nf, TB) / det;
            flat = !(fabs(det) >= kNormalMinDet) || !finite64(c[0]) || !finite64(c[1]) || !finite64(c[2]) || !(c[2] > 0.0);
            if (!flat) flat = !normalise3(c);
        }
    }
    if (flat) {
        c[0] = 0.0, c[1] = 0.0, c[2] = 1.0;
        flag |= kNormalFlat;
    }
    // 5. the bytes
#pragma unroll
    for (int k = 0; k < 3; k++) out[k] = raster_byte(127.5 * (c[k] + 1.0));
    offset[g] = canonical(s);
    flags[g] = (uint8_t)flag;
#pragma unroll
    for (int k = 0; k < 3; k++) normal[g * 3 + k] = canonical(Nf[k]);
}

struct LitCamera {
    double M[9];               // the ray direction of pixel (column j, row i) in body space: M (j, i, 1)
};

// Section 7k's headlight: clamp01(-n.d / |d|) as a float32, then image.to_8b_image's byte (a NaN gives 0).
__device__ __forceinline__ uint8_t headlight(const double nrm[3], const double d[3]) {
    const float v = (float)((-dot3(nrm, d)) / sqrt(dot3(d, d)));
    const float u = v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f;
    return (uint8_t)(int)(255.0f * u);
}

__global__ __launch_bounds__(kTexThreads) void mesh_resolve_lit_kernel(
    const unsigned long long *__restrict__ keys, const int32_t *__restrict__ faces, int64_t T, int64_t V,
    const int32_t *__restrict__ xy, const double *__restrict__ z, int H, int W, const float *__restrict__ vnormals,
    const float *__restrict__ tangents, const uint8_t *__restrict__ atlas, int aW, int n, int C, LitCamera cam, RasterBg bg,
    uint8_t *__restrict__ shade_geometry, uint8_t *__restrict__ shade_mapped) {
    const int64_t pix = (int64_t)blockIdx.x * kTexThreads + threadIdx.x;
    if (pix >= (int64_t)H * W) return;
    uint8_t geo[3] = {bg.c[0], bg.c[1], bg.c[2]}, map[3] = {bg.c[0], bg.c[1], bg.c[2]};
    ScreenWinner win;
    if (screen_winner(keys[pix], faces, T, V, xy, z, pix, W, win)) {
        const int64_t t = win.t;
        // the interpolated corner normal and tangent
        double N0[3], N1[3], N2[3], Nh[3], T0[3], T1[3], T2[3], Th[3], B[3], d[3];
        load3(vnormals + (int64_t)win.v0 * 3, N0), load3(vnormals + (int64_t)win.v1 * 3, N1), load3(vnormals + (int64_t)win.v2 * 3, N2);
        load3(tangents + (t * 3) * 4, T0), load3(tangents + (t * 3 + 1) * 4, T1), load3(tangents + (t * 3 + 2) * 4, T2);
        blend3(win.w0, win.w1, win.w2, N0, N1, N2, Nh);
        blend3(win.w0, win.w1, win.w2, T0, T1, T2, Th);
        const bool okN = normalise3(Nh), okT = normalise3(Th);
        const double dc = (double)win.col, dr = (double)win.row;
#pragma unroll
        for (int k = 0; k < 3; k++) d[k] = (cam.M[k * 3] * dc + cam.M[k * 3 + 1] * dr) + cam.M[k * 3 + 2];
        const double nanv[3] = {__longlong_as_double(0x7FF8000000000000ll), 0.0, 0.0};
        geo[0] = geo[1] = geo[2] = headlight(okN ? Nh : nanv, d);
        // the normal atlas through section 7o's sampler, the blend kept unrounded
        const AtlasTaps taps = atlas_taps(atlas, aW, t, win.w1, win.w2, n, C);
        double c[3];
        bool flat = true;                 // four taps of the flat code (128, 128, 255): the geometry's normal itself
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint8_t code = k == 2 ? 255 : 128;
            flat = flat && taps.c00[k] == code && taps.c10[k] == code && taps.c01[k] == code && taps.c11[k] == code;
            c[k] = taps.blend(k) / 127.5 - 1.0;
        }
        if (flat) {
            map[0] = map[1] = map[2] = geo[0];
        } else {
            double m[3];
            cross3(Nh, Th, B);
#pragma unroll
            for (int k = 0; k < 3; k++) m[k] = (c[0] * Th[k] + c[1] * B[k]) + c[2] * Nh[k];
            const bool okM = okN && okT && normalise3(m);
            map[0] = map[1] = map[2] = headlight(okM ? m : nanv, d);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) shade_geometry[pix * 3 + k] = geo[k], shade_mapped[pix * 3 + k] = map[k];
}

}  // namespace occ

OCC_API int occnerf_mesh_normal_bake(const float *verts, const float *vnormals, int64_t V, const int32_t *faces, int64_t T,
                                     const float *tangents, const uint8_t *creased, const float *pts, int32_t n, int32_t C,
                                     int32_t H, int32_t W, const float *field, int32_t nx, int32_t ny, int32_t nz,
                                     const double *h_lo, double h_f, float level, int32_t S, uint8_t *atlas, float *offset,
                                     uint8_t *flags, float *normal, int32_t *status, void *stream) {
    using namespace occ;
    if (!tex_cell_ok("mesh_normal_bake", n)) return 1;
    OCC_REQUIRE(V >= 0 && V < (1ll << 31), "mesh_normal_bake: V=%lld outside 0..2^31-1", (long long)V);
    int64_t P;
    if (!tex_count_ok("mesh_normal_bake", T, n, P) || !tex_atlas_ok("mesh_normal_bake", T, n, C, H, W)) return 1;
    OCC_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2 && (int64_t)nx * ny * nz < (1ll << 31),
                "mesh_normal_bake: a grid of %d x %d x %d points: every axis needs two, all of them fewer than 2^31", nx, ny, nz);
    OCC_REQUIRE(S >= 1 && S <= kNormalMaxSteps, "mesh_normal_bake: S=%d steps outside 1..%d", S, kNormalMaxSteps);
    OCC_REQUIRE(h_f > 0.0 && h_f <= kFiniteMax, "mesh_normal_bake: h_f=%g is not a positive finite voxel edge", h_f);
    if (T == 0) return 0;
    OCC_REQUIRE(faces && tangents && creased && pts && field && h_lo && atlas && offset && flags && normal && status &&
                ((verts && vnormals) || V == 0), "mesh_normal_bake: null argument");
    NormalGrid G;
    G.nx = nx, G.ny = ny, G.nz = nz;
    for (int k = 0; k < 3; k++) G.lo[k] = h_lo[k];
    G.h = h_f, G.level = (double)level, G.delta = h_f / 2.0, G.S = S;
    const int64_t N = T * P;
    hipLaunchKernelGGL(mesh_normal_bake_kernel, dim3((unsigned)((N + kTexThreads - 1) / kTexThreads)), dim3(kTexThreads), 0,
                       as_stream(stream), verts, vnormals, V, faces, T, tangents, creased, pts, (int)n, (int)P, (int)C, (int)W, field,
                       G, atlas, offset, flags, normal, status);
    return check_launch("mesh_normal_bake");
}

OCC_API int occnerf_mesh_resolve_lit(const uint64_t *keys, const int32_t *faces, int64_t T, int64_t V, const int32_t *xy,
                                     const double *z, int32_t Himg, int32_t Wimg, const float *vnormals, const float *tangents,
                                     const uint8_t *atlas, int32_t aH, int32_t aW, int32_t n, int32_t C, const double *h_M,
                                     const uint8_t *h_bgcolor, uint8_t *shade_geometry, uint8_t *shade_mapped, void *stream) {
    using namespace occ;
    OCC_REQUIRE(h_bgcolor && h_M, "mesh_resolve_lit: null argument");
    OCC_REQUIRE(raster_size_ok(Himg, Wimg), "mesh_resolve_lit: H=%d W=%d outside 1..16384 or more than 2^28 pixels", Himg, Wimg);
    if (!tex_cell_ok("mesh_resolve_lit", n)) return 1;
    OCC_REQUIRE(T >= 0 && T < (1ll << 31), "mesh_resolve_lit: T=%lld outside 0..2^31-1", (long long)T);
    OCC_REQUIRE(V >= 0 && V < (1ll << 31), "mesh_resolve_lit: V=%lld outside 0..2^31-1", (long long)V);
    OCC_REQUIRE(keys && shade_geometry && shade_mapped, "mesh_resolve_lit: null argument");
    if (T > 0 && V > 0) {
        if (!tex_atlas_ok("mesh_resolve_lit", T, n, C, aH, aW)) return 1;
        OCC_REQUIRE(faces && xy && z && vnormals && tangents && atlas, "mesh_resolve_lit: null argument");
    }
    LitCamera cam;
    for (int k = 0; k < 9; k++) cam.M[k] = h_M[k];
    RasterBg bg;
    for (int c = 0; c < 3; c++) bg.c[c] = h_bgcolor[c];
    const int64_t N = (int64_t)Himg * Wimg;
    const int64_t Tk = (T > 0 && V > 0) ? T : 0;      // no triangle: no key names one, the background everywhere
    hipLaunchKernelGGL(mesh_resolve_lit_kernel, dim3((unsigned)((N + kTexThreads - 1) / kTexThreads)), dim3(kTexThreads), 0,
                       as_stream(stream), (const unsigned long long *)keys, faces, Tk, V, xy, z, (int)Himg, (int)Wimg, vnormals,
                       tangents, atlas, (int)aW, (int)n, (int)C, cam, bg, shade_geometry, shade_mapped);
    return check_launch("mesh_resolve_lit");
}
