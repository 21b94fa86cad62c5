// The geometry the volume renderer sees, per pixel (no counterpart in the reference, which drops the
// compositor's depth): the surface point of every ray from its composited depth, a normal from the secants to the
// neighbouring pixels' points, and the depth / normal / shaded panels as 8-bit pixels.  Two launches, one thread per pixel,
// no atomics: the bytes are a pure function of the inputs, bit-identical to tests/gbuffer_restatement.py (float32, one
// rounding per operator -- the tree is built with -ffp-contract=off -- __fdiv_rn and sqrtf correctly rounded).
//
// Launch 1 finds the pixel's ray by the binary search of assemble_image_kernel (image.hip) and leaves the ray's row in a
// pixel -> ray column, -1 where the pixel has no ray or its depth is not valid; launch 2 takes its neighbours' validity and
// its own direction from that column (4 B per pixel, coalesced) instead of searching again, and is the only writer of the
// final valid byte, so no thread reads a byte another one writes.  Bound: HBM streaming; the point map (16 B per pixel,
// float4 stores and loads) is L2-resident at 512 x 512.  The [R,3] ray rows and the [H,W,3] outputs are 12-byte records:
// their layout is the caller's (the renderer's rays, numpy's images), so they move as three dwords per lane.
#include "batch_common.h"

namespace occ {

struct GbufferParams {
    float bg[3];       // cfg.bgcolor / 255 as float32, like ImageParams
};

__device__ __forceinline__ bool finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// min(max(x, 0), 1) with NaN -> 0: the greys of the depth and shaded panels.
__device__ __forceinline__ float clamp01(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }

__global__ __launch_bounds__(256) void gbuffer_points_kernel(const int64_t *__restrict__ ray_index, int64_t R,
                                                             const float *__restrict__ rays, const float *__restrict__ depth,
                                                             const float *__restrict__ alpha, float min_alpha, int64_t n_pixels,
                                                             float4 *__restrict__ points, uint8_t *__restrict__ valid,
                                                             int32_t *__restrict__ pix_ray) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    int64_t lo = 0, hi = R;                                 // first ray with ray_index >= p
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ray_index[mid] < p) lo = mid + 1;
        else hi = mid;
    }
    float4 P = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int32_t row = -1;
    if (lo < R && ray_index[lo] == p) {
        const float a = alpha[lo], z = depth[lo];
        if (a >= min_alpha && a > 0.0f && finite_f32(a) && finite_f32(z)) {
            const float t = __fdiv_rn(z, a);                // the compositor's depth is not normalised by the weight sum
            P.x = __fadd_rn(rays[lo * 3], __fmul_rn(t, rays[(R + lo) * 3]));
            P.y = __fadd_rn(rays[lo * 3 + 1], __fmul_rn(t, rays[(R + lo) * 3 + 1]));
            P.z = __fadd_rn(rays[lo * 3 + 2], __fmul_rn(t, rays[(R + lo) * 3 + 2]));
            P.w = t;
            row = (int32_t)lo;                              // R <= H * W < 2^31
        }
    }
    points[p] = P;
    valid[p] = row >= 0 ? 1 : 0;
    pix_ray[p] = row;
}

// The secant along one image axis: `fwd` / `bwd` say whether the neighbour after / before the pixel is inside the image and
// depth-valid (Pf / Pb are read only then).  The candidate with the smaller |dt| wins, a tie goes to the forward one.
__device__ __forceinline__ bool secant(const float4 &P, bool fwd, const float4 &Pf, bool bwd, const float4 &Pb, float (&s)[3]) {
    const bool use_b = bwd && (!fwd || fabsf(__fsub_rn(P.w, Pb.w)) < fabsf(__fsub_rn(Pf.w, P.w)));
    if (use_b) {
        s[0] = __fsub_rn(P.x, Pb.x);
        s[1] = __fsub_rn(P.y, Pb.y);
        s[2] = __fsub_rn(P.z, Pb.z);
    } else if (fwd) {
        s[0] = __fsub_rn(Pf.x, P.x);
        s[1] = __fsub_rn(Pf.y, P.y);
        s[2] = __fsub_rn(Pf.z, P.z);
    }
    return fwd || bwd;
}

__device__ __forceinline__ void store_grey(uint8_t *out, int64_t p, uint8_t q) {
    out[p * 3] = q;
    out[p * 3 + 1] = q;
    out[p * 3 + 2] = q;
}

__global__ __launch_bounds__(256) void gbuffer_normals_kernel(const float4 *__restrict__ points, const int32_t *__restrict__ pix_ray,
                                                              const float *__restrict__ rays, int64_t R, int32_t H, int32_t W,
                                                              const float *__restrict__ t_range, GbufferParams prm,
                                                              float *__restrict__ normal, uint8_t *__restrict__ valid,
                                                              uint8_t *__restrict__ depth_u8, uint8_t *__restrict__ normal_u8,
                                                              uint8_t *__restrict__ shaded_u8) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const int32_t i = (int32_t)(p / W), j = (int32_t)(p - (int64_t)i * W);
    const int32_t row = pix_ray[p];
    const bool dv = row >= 0 && row < R;                    // a column that is not launch 1's is never used as an address
    float n[3] = {0.0f, 0.0f, 0.0f}, shade = 0.0f, t = 0.0f;
    bool nv = false;
    if (dv) {
        const float4 P = points[p];
        t = P.w;
        float4 Pf = P, Pb = P;
        float a[3] = {0.0f, 0.0f, 0.0f}, b[3] = {0.0f, 0.0f, 0.0f};
        bool fwd = j + 1 < W && pix_ray[p + 1] >= 0, bwd = j > 0 && pix_ray[p - 1] >= 0;
        if (fwd) Pf = points[p + 1];
        if (bwd) Pb = points[p - 1];
        const bool has_a = secant(P, fwd, Pf, bwd, Pb, a);
        fwd = i + 1 < H && pix_ray[p + W] >= 0;
        bwd = i > 0 && pix_ray[p - W] >= 0;
        if (fwd) Pf = points[p + W];
        if (bwd) Pb = points[p - W];
        const bool has_b = secant(P, fwd, Pf, bwd, Pb, b);
        if (has_a && has_b) {
            const float d0 = rays[(R + row) * 3], d1 = rays[(R + row) * 3 + 1], d2 = rays[(R + row) * 3 + 2];
            n[0] = __fsub_rn(__fmul_rn(a[1], b[2]), __fmul_rn(a[2], b[1]));
            n[1] = __fsub_rn(__fmul_rn(a[2], b[0]), __fmul_rn(a[0], b[2]));
            n[2] = __fsub_rn(__fmul_rn(a[0], b[1]), __fmul_rn(a[1], b[0]));
            const float s = __fadd_rn(__fadd_rn(__fmul_rn(n[0], d0), __fmul_rn(n[1], d1)), __fmul_rn(n[2], d2));
            if (s > 0.0f) {                                 // towards the camera
                n[0] = -n[0];
                n[1] = -n[1];
                n[2] = -n[2];
            }
            const float l2 = __fadd_rn(__fadd_rn(__fmul_rn(n[0], n[0]), __fmul_rn(n[1], n[1])), __fmul_rn(n[2], n[2]));
            nv = finite_f32(l2) && l2 != 0.0f;
            if (nv) {
                const float l = sqrtf(l2);
                n[0] = __fdiv_rn(n[0], l);
                n[1] = __fdiv_rn(n[1], l);
                n[2] = __fdiv_rn(n[2], l);
                const float nd = __fadd_rn(__fadd_rn(__fmul_rn(n[0], d0), __fmul_rn(n[1], d1)), __fmul_rn(n[2], d2));
                const float dd = __fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2));
                shade = clamp01(__fdiv_rn(-nd, sqrtf(dd)));  // a headlight: the cosine between the normal and the ray back
            } else {
                n[0] = n[1] = n[2] = 0.0f;
            }
        }
    }
    normal[p * 3] = n[0];
    normal[p * 3 + 1] = n[1];
    normal[p * 3 + 2] = n[2];
    valid[p] = (uint8_t)((dv ? 1 : 0) | (nv ? 2 : 0));
    const uint8_t bg0 = to_8b(prm.bg[0]), bg1 = to_8b(prm.bg[1]), bg2 = to_8b(prm.bg[2]);
    if (depth_u8) {
        if (dv) {
            const float t_lo = t_range[0], t_hi = t_range[1];
            store_grey(depth_u8, p, to_8b(clamp01(__fdiv_rn(__fsub_rn(t_hi, t), __fsub_rn(t_hi, t_lo)))));
        } else {
            depth_u8[p * 3] = bg0;
            depth_u8[p * 3 + 1] = bg1;
            depth_u8[p * 3 + 2] = bg2;
        }
    }
    if (normal_u8) {
        normal_u8[p * 3] = nv ? to_8b(__fadd_rn(__fmul_rn(0.5f, n[0]), 0.5f)) : bg0;
        normal_u8[p * 3 + 1] = nv ? to_8b(__fadd_rn(__fmul_rn(0.5f, n[1]), 0.5f)) : bg1;
        normal_u8[p * 3 + 2] = nv ? to_8b(__fadd_rn(__fmul_rn(0.5f, n[2]), 0.5f)) : bg2;
    }
    if (shaded_u8) {
        if (nv) {
            store_grey(shaded_u8, p, to_8b(shade));
        } else {
            shaded_u8[p * 3] = bg0;
            shaded_u8[p * 3 + 1] = bg1;
            shaded_u8[p * 3 + 2] = bg2;
        }
    }
}

constexpr int64_t kGbufferMaxPixels = (int64_t)1 << 31;     // the pixel -> ray column is int32

}  // namespace occ

OCC_API int occnerf_gbuffer_points(const int64_t *ray_index, int64_t R, const float *rays, const float *depth,
                                   const float *alpha, float min_alpha, int32_t height, int32_t width, float *points,
                                   uint8_t *valid, int32_t *pix_ray, void *stream) {
    using namespace occ;
    OCC_REQUIRE(height > 0 && width > 0 && R >= 0 && (int64_t)height * width < kGbufferMaxPixels, "gbuffer_points: bad sizes");
    OCC_REQUIRE(R <= (int64_t)height * width, "gbuffer_points: R = %lld is larger than height * width = %lld", (long long)R,
                (long long)height * width);
    OCC_REQUIRE(points && valid && pix_ray && (R == 0 || (ray_index && rays && depth && alpha)), "gbuffer_points: null argument");
    const int64_t n = (int64_t)height * width;
    hipLaunchKernelGGL(gbuffer_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), ray_index, R,
                       rays, depth, alpha, min_alpha, n, reinterpret_cast<float4 *>(points), valid, pix_ray);
    return check_launch("gbuffer_points");
}

OCC_API int occnerf_gbuffer_normals(const float *points, const int32_t *pix_ray, const float *rays, int64_t R, int32_t height,
                                    int32_t width, const float *t_range, const float *h_bgcolor01, float *normal,
                                    uint8_t *valid, uint8_t *depth_u8, uint8_t *normal_u8, uint8_t *shaded_u8, void *stream) {
    using namespace occ;
    OCC_REQUIRE(height > 0 && width > 0 && R >= 0 && (int64_t)height * width < kGbufferMaxPixels, "gbuffer_normals: bad sizes");
    OCC_REQUIRE(R <= (int64_t)height * width, "gbuffer_normals: R = %lld is larger than height * width = %lld", (long long)R,
                (long long)height * width);
    OCC_REQUIRE(points && pix_ray && h_bgcolor01 && normal && valid && (R == 0 || rays) && (!depth_u8 || t_range),
                "gbuffer_normals: null argument");
    GbufferParams prm;
    for (int c = 0; c < 3; c++) prm.bg[c] = h_bgcolor01[c];
    const int64_t n = (int64_t)height * width;
    hipLaunchKernelGGL(gbuffer_normals_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const float4 *>(points), pix_ray, rays, R, height, width, t_range, prm, normal, valid,
                       depth_u8, normal_u8, shaded_u8);
    return check_launch("gbuffer_normals");
}
