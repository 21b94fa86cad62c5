// The exported mesh as a rig (occnerf_amd/mesh.py skin_mesh / export_rig): the motion-weight volume read
// as the skinning field of the canonical mesh, and the forward linear blend skinning that field defines.
//
//   mesh_skin   per canonical vertex the K largest positive taps of the bones' channels at the vertex itself (descending, ties:
//               the lower index), normalised over the kept ones.  One thread per vertex; the list of the K best is K doubles and
//               K ints kept sorted by an unrolled insertion, every array indexed by unrolled constants only: nothing is spilled.
//   mesh_lbs    p = sum_k w_k R_b^T (x - T_b) for F frames at once, grid (vertex blocks, F), the frame's transforms staged in
//               LDS once per workgroup; with targets also the displacement d with M d = target - p, M = sum_k w_k R_b^T, by
//               Cramer's rule: the morph target that makes the skinned vertex land on the target.
//
// fp64 with + - * / floor and comparisons only, one rounding per operator in the order of tests/mesh_rig_restatement.py (the
// tree is built with -ffp-contract=off): the outputs are that file's, bit for bit.  No atomics; pure functions of the inputs.
// The tap is that of mesh_pose.hip (tests/mesh_pose_restatement.py canonical_weights).
#include "common.h"

namespace occ {

constexpr int kRigMaxBones = 32;
constexpr int kRigThreads = 256;

struct RigParams {
    float bmin[3];
    float bscale[3];
};

template <int K>
__global__ __launch_bounds__(kRigThreads) void mesh_skin_kernel(
    const float *__restrict__ x_c, int64_t V, const float *__restrict__ vol, int nb, int G, RigParams prm,
    uint8_t *__restrict__ joints, float *__restrict__ weights, uint8_t *__restrict__ count, float *__restrict__ kept) {
    const int64_t i = (int64_t)blockIdx.x * kRigThreads + threadIdx.x;
    if (i >= V) return;
    const double gm1 = (double)(G - 1);
    double w0[3], w1[3];
    int i0[3];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double g = ((double)x_c[i * 3 + c] - (double)prm.bmin[c]) * (double)prm.bscale[c] - 1.0;
        const double ix = ((g + 1.0) / 2.0) * gm1;
        const double f = floor(ix);
        ok = ok && f >= -1.0 && f <= gm1;      // (false for NaN)
        w1[c] = ix - f;
        w0[c] = (f + 1.0) - ix;
        i0[c] = (f >= -1.0 && f <= gm1) ? (int)f : 0;
    }
    double cs[K], total = 0.0;
    int js[K];
#pragma unroll
    for (int k = 0; k < K; k++) cs[k] = 0.0, js[k] = 0;
    if (ok) {
        const size_t vsz = (size_t)G * G * G;
#pragma unroll 1
        for (int b = 0; b < nb; b++) {
            const float *__restrict__ volb = vol + (size_t)b * vsz;
            double c = 0.0;
#pragma unroll
            for (int t = 0; t < 8; t++) {
                const int x = i0[0] + (t & 1), y = i0[1] + ((t >> 1) & 1), z = i0[2] + (t >> 2);
                const bool in = x >= 0 && x < G && y >= 0 && y < G && z >= 0 && z < G;
                const double v = in ? (double)volb[((size_t)z * G + y) * G + x] : 0.0;
                const double wx = (t & 1) ? w1[0] : w0[0], wy = ((t >> 1) & 1) ? w1[1] : w0[1], wz = (t >> 2) ? w1[2] : w0[2];
                c = c + v * ((wx * wy) * wz);
            }
            total = total + c;
            // sorted insertion: behind every entry that is at least as large (an earlier bone wins a tie), the rest moves down
            double cv = c;
            int jv = b;
            bool moving = false;
#pragma unroll
            for (int k = 0; k < K; k++) {
                if (moving || cv > cs[k]) {
                    const double tc = cs[k];
                    const int tj = js[k];
                    cs[k] = cv, js[k] = jv;
                    cv = tc, jv = tj;
                    moving = true;
                }
            }
        }
    }
    int n = 0;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < K; k++) {
        n += cs[k] > 0.0 ? 1 : 0;
        s = s + cs[k];
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
        const bool used = cs[k] > 0.0;
        joints[i * K + k] = (uint8_t)(used ? js[k] : 0);
        weights[i * K + k] = used ? (float)(cs[k] / s) : ((n == 0 && k == 0) ? 1.0f : 0.0f);
    }
    count[i] = (uint8_t)n;
    kept[i] = n ? (float)(s / total) : 0.0f;
}

template <int K, bool kTarget>
__global__ __launch_bounds__(kRigThreads) void mesh_lbs_kernel(
    const float *__restrict__ x_c, int64_t V, const uint8_t *__restrict__ joints, const float *__restrict__ weights,
    const float *__restrict__ Rs, const float *__restrict__ Ts, int nb, const float *__restrict__ target,
    const uint8_t *__restrict__ target_flag, double max_delta, float *__restrict__ posed, float *__restrict__ delta,
    uint8_t *__restrict__ dflag) {
    __shared__ float sR[kRigMaxBones * 9];
    __shared__ float sT[kRigMaxBones * 3];
    const size_t f = blockIdx.y;
    for (int t = threadIdx.x; t < nb * 9; t += blockDim.x) sR[t] = Rs[f * (size_t)nb * 9 + t];
    for (int t = threadIdx.x; t < nb * 3; t += blockDim.x) sT[t] = Ts[f * (size_t)nb * 3 + t];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kRigThreads + threadIdx.x;
    if (i >= V) return;
    const double x0 = (double)x_c[i * 3], x1 = (double)x_c[i * 3 + 1], x2 = (double)x_c[i * 3 + 2];
    double p[3] = {0.0, 0.0, 0.0}, M[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < K; k++) {
        const double w = (double)weights[i * K + k];
        const int b = joints[i * K + k];
        if (w != 0.0 && b < nb) {          // (the wrapper refuses a joint index >= nb; it is never used as an address)
            const double d0 = x0 - (double)sT[b * 3], d1 = x1 - (double)sT[b * 3 + 1], d2 = x2 - (double)sT[b * 3 + 2];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double r0 = (double)sR[b * 9 + j], r1 = (double)sR[b * 9 + 3 + j], r2 = (double)sR[b * 9 + 6 + j];
                const double q = (r0 * d0 + r1 * d1) + r2 * d2;
                p[j] = p[j] + w * q;
                if (kTarget) {
                    M[j * 3] = M[j * 3] + w * r0;
                    M[j * 3 + 1] = M[j * 3 + 1] + w * r1;
                    M[j * 3 + 2] = M[j * 3 + 2] + w * r2;
                }
            }
        }
    }
    const size_t o = f * (size_t)V + (size_t)i;
#pragma unroll
    for (int c = 0; c < 3; c++) posed[o * 3 + c] = (float)p[c];
    if (kTarget) {
        const double n0 = (double)target[o * 3] - p[0], n1 = (double)target[o * 3 + 1] - p[1], n2 = (double)target[o * 3 + 2] - p[2];
        const double m_ei = M[4] * M[8] - M[5] * M[7], m_di = M[3] * M[8] - M[5] * M[6], m_dh = M[3] * M[7] - M[4] * M[6];
        const double det = (M[0] * m_ei - M[1] * m_di) + M[2] * m_dh;
        const double q1 = n1 * M[8] - M[5] * n2, q2 = n1 * M[7] - M[4] * n2, q3 = M[3] * n2 - n1 * M[6];
        const double e0 = ((n0 * m_ei - M[1] * q1) + M[2] * q2) / det;
        const double e1 = ((M[0] * q1 - n0 * m_di) + M[2] * q3) / det;
        const double e2 = ((M[0] * (M[4] * n2 - n1 * M[7]) - M[1] * q3) + n0 * m_dh) / det;
        const bool solved = det != 0.0 && fabs(det) <= 1.7976931348623157e308 && target_flag[o] == 0 &&
                            fabs(e0) <= max_delta && fabs(e1) <= max_delta && fabs(e2) <= max_delta;      // (false for NaN)
        delta[o * 3] = solved ? (float)e0 : 0.0f;
        delta[o * 3 + 1] = solved ? (float)e1 : 0.0f;
        delta[o * 3 + 2] = solved ? (float)e2 : 0.0f;
        dflag[o] = solved ? 0 : 1;
    }
}

}  // namespace occ

OCC_API int occnerf_mesh_skin(const float *x_c, int64_t V, const float *vol, int32_t nb, int32_t G, const float *h_bbox_min,
                              const float *h_bbox_scale, int32_t K, uint8_t *joints, float *weights, uint8_t *count, float *kept,
                              void *stream) {
    using namespace occ;
    OCC_REQUIRE(vol && h_bbox_min && h_bbox_scale, "mesh_skin: null argument");
    OCC_REQUIRE(K == 4 || K == 8, "mesh_skin: K=%d is neither 4 nor 8", K);
    OCC_REQUIRE(nb >= 1 && nb <= kRigMaxBones, "mesh_skin: nb=%d outside 1..%d", nb, kRigMaxBones);
    OCC_REQUIRE(G >= 2 && G <= 1024, "mesh_skin: G=%d outside 2..1024", G);
    OCC_REQUIRE(V >= 0 && V < (1ll << 31) * kRigThreads, "mesh_skin: V=%lld out of range", (long long)V);
    if (V == 0) return 0;
    OCC_REQUIRE(x_c && joints && weights && count && kept, "mesh_skin: null x_c / output with V=%lld", (long long)V);
    RigParams prm;
    for (int c = 0; c < 3; c++) {
        prm.bmin[c] = h_bbox_min[c];
        prm.bscale[c] = h_bbox_scale[c];
    }
    const dim3 grid((unsigned)((V + kRigThreads - 1) / kRigThreads)), block(kRigThreads);
    if (K == 4)
        hipLaunchKernelGGL(mesh_skin_kernel<4>, grid, block, 0, as_stream(stream), x_c, V, vol, nb, G, prm, joints, weights, count,
                           kept);
    else
        hipLaunchKernelGGL(mesh_skin_kernel<8>, grid, block, 0, as_stream(stream), x_c, V, vol, nb, G, prm, joints, weights, count,
                           kept);
    return check_launch("mesh_skin");
}

OCC_API int occnerf_mesh_lbs(const float *x_c, int64_t V, const uint8_t *joints, const float *weights, int32_t K, const float *Rs,
                             const float *Ts, int32_t F, int32_t nb, const float *target, const uint8_t *target_flag,
                             double max_delta, float *posed, float *delta, uint8_t *dflag, void *stream) {
    using namespace occ;
    OCC_REQUIRE(Rs && Ts, "mesh_lbs: null argument");
    OCC_REQUIRE(F >= 1 && F <= 65535, "mesh_lbs: F=%d outside 1..65535", F);
    OCC_REQUIRE(K == 4 || K == 8, "mesh_lbs: K=%d is neither 4 nor 8", K);
    OCC_REQUIRE(nb >= 1 && nb <= kRigMaxBones, "mesh_lbs: nb=%d outside 1..%d", nb, kRigMaxBones);
    OCC_REQUIRE(max_delta >= 0.0 && max_delta <= 1.7976931348623157e308, "mesh_lbs: max_delta=%g must be a finite number >= 0",
                max_delta);
    OCC_REQUIRE(V >= 0 && V < (1ll << 31), "mesh_lbs: V=%lld out of range", (long long)V);
    if (V == 0) return 0;
    OCC_REQUIRE(x_c && joints && weights && posed, "mesh_lbs: null x_c / joints / weights / posed with V=%lld", (long long)V);
    OCC_REQUIRE(!target || (target_flag && delta && dflag), "mesh_lbs: null target_flag / delta / dflag with a target");
    const dim3 grid((unsigned)((V + kRigThreads - 1) / kRigThreads), (unsigned)F), block(kRigThreads);
#define OCC_LBS(KK, TT)                                                                                                      \
    hipLaunchKernelGGL((mesh_lbs_kernel<KK, TT>), grid, block, 0, as_stream(stream), x_c, V, joints, weights, Rs, Ts, nb, target, \
                       target_flag, max_delta, posed, delta, dflag)
    if (K == 4 && target) OCC_LBS(4, true);
    else if (K == 4) OCC_LBS(4, false);
    else if (target) OCC_LBS(8, true);
    else OCC_LBS(8, false);
#undef OCC_LBS
    return check_launch("mesh_lbs");
}
