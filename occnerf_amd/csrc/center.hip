// Collapsed samples, classified once in front of the kNN and feature kernels.
//
// Two thirds of a frame's live samples land, after the non-rigid offset, within the radius around the frame's collapse
// point c in which c's neighbour lists provably hold (csrc/knn.hip: the centre cache).  For such a sample the kNN kernel
// hands out c's 40 ids, the feature kernel's columns 0..35 are c's (functions of the ids, the table and the counters alone),
// and when its encoder input x[4] is bitwise c's the 32 encoded columns are c's as well: its whole mlp_in row is the
// centre row.  center_classify_kernel finds those samples with one lane each -- the inside test of the two kernels and the
// feature kernel's geometry phase on c's ten finest neighbours, whose records are wave-uniform here -- and writes their
// signed distance; occnerf_center_split (csrc/compact.hip) takes them out of the list the kNN and feature kernels see.
//
// The arithmetic is the feature kernel's, operation for operation and in its order (csrc/features.hip,
// sample_features8_kernel): every flagged sample's x and distance carry the bits that kernel would have produced.
#include "common.h"

namespace occ {

constexpr int kKnn = 10;

// csrc/features.hip cos3_unit: F.cosine_similarity(float32 dir, float64 normal) with the pre-normalised fp64 normal
__device__ __forceinline__ double cos3_unit(const float (&a)[3], const double (&un)[3]) {
    float na = norm3(a[0], a[1], a[2]);
    na = na < 1e-8f ? 1e-8f : na;
    const double t0 = __dmul_rn((double)__fdiv_rn(a[0], na), un[0]);
    const double t1 = __dmul_rn((double)__fdiv_rn(a[1], na), un[1]);
    const double t2 = __dmul_rn((double)__fdiv_rn(a[2], na), un[2]);
    return __dadd_rn(__dadd_rn(t0, t1), t2);
}

// 64-byte record of occnerf_point_pack: base xyz (fp32) + pad | normal x, y, z | unit normal x, y, z (fp64)
struct GeoRec {
    float base[3], pad;
    double normal[3], unit[3];
};
static_assert(sizeof(GeoRec) == 64, "GeoRec is the 64-byte record of occnerf_point_pack");

// One lane per entry o of the live list.  flag[o] = 1 iff the sample lies inside the centre's radius AND its encoder input
// is bitwise the centre's (center_agg[36..39]); raw_c[o*5+4] = its signed distance then.  The ten records are fetched
// through wave-uniform addresses (scalar loads); no LDS, no barrier, no atomic.
constexpr int kClassifyBlock = 256;      // (64 to 512 measured within 5 % of each other on the headline frame, 1 024 8 % behind: ~50 B streamed per sample)

__global__ __launch_bounds__(kClassifyBlock) void center_classify_kernel(
    const float *__restrict__ xyz, const int32_t *__restrict__ rows, const int32_t *__restrict__ n_dev,
    const GeoRec *__restrict__ geo, int P, const float *__restrict__ center, const int32_t *__restrict__ center_idx,
    const float *__restrict__ center_agg, float bound, float two_bound, uint8_t *__restrict__ flag,
    float *__restrict__ raw_c) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = (int64_t)*n_dev;
    if ((int64_t)blockIdx.x * blockDim.x >= n) return;               // uniform for the workgroup
    const bool live = o < n;
    const float ccx = center[0], ccy = center[1], ccz = center[2], cr2 = center[3];
    float p[3] = {0.f, 0.f, 0.f};
    bool inside = false;
    if (live) {
        const int64_t i = rows[o];
        struct __attribute__((packed, aligned(4))) F3 { float v[3]; };
        const F3 pq = *reinterpret_cast<const F3 *>(xyz + i * 3);
        p[0] = pq.v[0], p[1] = pq.v[1], p[2] = pq.v[2];
        const float dx = p[0] - ccx, dy = p[1] - ccy, dz = p[2] - ccz;
        inside = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)) < cr2;      // knn.hip / features.hip
    }
    bool take = false;
    if (inside) {                                                    // (a wave of outside samples skips the block)
        int neg = 0;
        float dsum = 0.0f;
        double num[3] = {0.0, 0.0, 0.0}, den = 0.0;
#pragma unroll
        for (int j = 0; j < kKnn; j++) {
            int id = center_idx[j];                                  // wave-uniform
            id = id < 0 ? 0 : (id >= P ? P - 1 : id);                // (the search returns ids in [0, P): never moves one)
            const GeoRec r = geo[id];
            float dir[3];
#pragma unroll
            for (int c = 0; c < 3; c++) dir[c] = __fsub_rn(p[c], r.base[c]);
            double dot = __dadd_rn(0.0, __dmul_rn((double)dir[0], r.normal[0]));
            dot = __dadd_rn(dot, __dmul_rn((double)dir[1], r.normal[1]));
            dot = __dadd_rn(dot, __dmul_rn((double)dir[2], r.normal[2]));
            neg += dot < 0.0;
            dsum = __fadd_rn(dsum, norm3(dir[0], dir[1], dir[2]));
            if (j < 3) {
                const double att = fabs(cos3_unit(dir, r.unit));
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float pn = __fdiv_rn(__fadd_rn(r.base[c], bound), two_bound);
                    num[c] = __dadd_rn(num[c], __dmul_rn(att, (double)pn));
                }
                den = __dadd_rn(den, att);
            }
        }
        float dist = __fdiv_rn(dsum, (float)kKnn);
        if (2 * neg > kKnn) dist = -dist;
        float nd = __fdiv_rn(__fadd_rn(dist, 0.2f), 0.5f);
        nd = nd < 0.0f ? 0.0f : (nd > 1.0f ? 1.0f : nd);
        float x[4];
#pragma unroll
        for (int c = 0; c < 3; c++) x[c] = (float)__ddiv_rn(num[c], den);
        x[3] = nd;
        take = inside && __float_as_uint(x[0]) == __float_as_uint(center_agg[36]) &&
               __float_as_uint(x[1]) == __float_as_uint(center_agg[37]) &&
               __float_as_uint(x[2]) == __float_as_uint(center_agg[38]) &&
               __float_as_uint(x[3]) == __float_as_uint(center_agg[39]);
        if (take) raw_c[o * 5 + 4] = dist;
    }
    if (live) flag[o] = take ? 1 : 0;
}

// raw_c[keep[o2]*5+4] = raw2[o2*5+4]: the kept samples' signed distance, from the feature kernel's compact rows back to
// their positions in the live list
__global__ void center_merge_dist_kernel(const float *__restrict__ raw2, const int32_t *__restrict__ keep,
                                         const int32_t *__restrict__ n2_dev, float *__restrict__ raw_c) {
    const int64_t o2 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o2 >= (int64_t)*n2_dev) return;
    raw_c[(int64_t)keep[o2] * 5 + 4] = raw2[o2 * 5 + 4];
}

}  // namespace occ

OCC_API int occnerf_center_classify(const float *xyz, const int32_t *rows, const int32_t *n_dev, int64_t N_max,
                                    const float *point_geo, int32_t P, const float *center, const int32_t *center_idx,
                                    const float *center_agg, float bound, float two_bound, uint8_t *flag, float *raw_c,
                                    void *stream) {
    using namespace occ;
    if (N_max <= 0) return 0;
    OCC_REQUIRE(xyz && rows && n_dev && point_geo && center && center_idx && center_agg && flag && raw_c,
                "center_classify: null argument");
    OCC_REQUIRE(P > 0, "center_classify: P=%d rows of packed point records", P);
    const int64_t blocks = (N_max + kClassifyBlock - 1) / kClassifyBlock;
    OCC_REQUIRE(blocks < (1ll << 31), "center_classify: N too large");
    hipLaunchKernelGGL(center_classify_kernel, dim3((unsigned)blocks), dim3(kClassifyBlock), 0, as_stream(stream), xyz, rows, n_dev,
                       reinterpret_cast<const GeoRec *>(point_geo), (int)P, center, center_idx, center_agg, bound, two_bound,
                       flag, raw_c);
    return check_launch("center_classify");
}

OCC_API int occnerf_center_merge_dist(const float *raw2, const int32_t *keep, const int32_t *n2_dev, int64_t N_max,
                                      float *raw_c, void *stream) {
    using namespace occ;
    if (N_max <= 0) return 0;
    OCC_REQUIRE(raw2 && keep && n2_dev && raw_c, "center_merge_dist: null argument");
    const int64_t blocks = (N_max + 255) / 256;
    OCC_REQUIRE(blocks < (1ll << 31), "center_merge_dist: N too large");
    hipLaunchKernelGGL(center_merge_dist_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), raw2, keep,
                       n2_dev, raw_c);
    return check_launch("center_merge_dist");
}
