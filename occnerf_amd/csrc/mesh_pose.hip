// The exported mesh in a frame's pose (occnerf_amd/mesh.py pose_mesh): per canonical vertex x_c the
// observation-space point p with F(p) = x_c, F the skeletal warp of warp.hip written out in fp64.  The model only knows the
// backward map, so every vertex runs a damped Newton iteration on F with the analytic Jacobian of the trilinear taps, started
// at the rigid inverse R_b^T (x_c - T_b) of the bone that owns the vertex in canonical space (the bones with a non-zero
// canonical weight, by descending weight, at most `candidates` of them).
//
// One thread per vertex, no MFMA: the work is the gather of 24 bones x 8 taps per evaluation from the 3.1 MB volume, which
// stays in L2.  Bone transforms are staged in LDS once per workgroup; the whole solver state (p, F, J, delta: 21 doubles, and
// the 16 accumulators of an evaluation) lives in registers: every array below is indexed by unrolled constants only, and the
// candidate list is never stored -- the next candidate is found by another pass over the bones' canonical weights, which runs
// only when a candidate has failed.  A bone whose tap lies off the grid contributes nothing and is skipped per lane.
//
// fp64 with + - * / floor and comparisons only, one rounding per operator in the order of tests/mesh_pose_restatement.py (the
// tree is built with -ffp-contract=off): the outputs are that file's, bit for bit.  No atomics; a pure function of the inputs.
#include "common.h"

namespace occ {

constexpr int kPoseMaxBones = 32;
constexpr int kPoseThreads = 256;
constexpr double kPoseClamp = 1e-4;

struct PoseParams {
    float bmin[3];
    float bscale[3];
};

struct PoseTap {
    bool ok;              // floor index inside [-1, G - 1] on every axis: at least one corner can be on the grid
    int i0[3];            // floor index per axis (x, y, z)
    double w0[3], w1[3];  // weight of the lower / upper corner per axis
};

__device__ __forceinline__ PoseTap pose_tap(const double (&pos)[3], const double (&bmin)[3], const double (&bscale)[3], int G) {
    PoseTap t;
    const double gm1 = (double)(G - 1);
    double f[3];
    t.ok = true;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double g = (pos[c] - bmin[c]) * bscale[c] - 1.0;
        const double ix = ((g + 1.0) / 2.0) * gm1;
        f[c] = floor(ix);
        t.ok = t.ok && f[c] >= -1.0 && f[c] <= gm1;      // (false for NaN)
        t.w1[c] = ix - f[c];
        t.w0[c] = (f[c] + 1.0) - ix;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) t.i0[c] = t.ok ? (int)f[c] : 0;
    return t;
}

// The eight corner values v[dz * 4 + dy * 2 + dx] of one bone's channel, 0 where the corner is off the grid (never read).
__device__ __forceinline__ void pose_corners(const float *__restrict__ volb, int G, const PoseTap &t, double (&v)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int x = t.i0[0] + (i & 1), y = t.i0[1] + ((i >> 1) & 1), z = t.i0[2] + (i >> 2);
        const bool in = x >= 0 && x < G && y >= 0 && y < G && z >= 0 && z < G;
        v[i] = in ? (double)volb[((size_t)z * G + y) * G + x] : 0.0;
    }
}

__device__ __forceinline__ double pose_weight(const PoseTap &t, const double (&v)[8]) {
    double out = 0.0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const double wx = (i & 1) ? t.w1[0] : t.w0[0], wy = ((i >> 1) & 1) ? t.w1[1] : t.w0[1], wz = (i >> 2) ? t.w1[2] : t.w0[2];
        out = out + v[i] * ((wx * wy) * wz);
    }
    return out;
}

__device__ __forceinline__ double pose_norm(const double (&F)[3], const double (&x)[3]) {
    const double a0 = fabs(F[0] - x[0]), a1 = fabs(F[1] - x[1]), a2 = fabs(F[2] - x[2]);
    const double m = a1 > a0 ? a1 : a0;
    return a2 > m ? a2 : m;
}

struct PoseFrame {
    const float *sR, *sT;         // LDS: nb x 9, nb x 3
    const float *vol;
    int nb, G;
    size_t vsz;
    double bmin[3], bscale[3], k[3];      // k = bscale * (G - 1) / 2: d(grid index) / d(position)
};

// F(p), sum of the weights and (kJac) the Jacobian dF/dp, row-major J[a * 3 + j] = dF_a / dp_j.
template <bool kJac>
__device__ __forceinline__ void pose_eval(const PoseFrame &fr, const double (&p)[3], double (&F)[3], double &wsum_out,
                                          double (&J)[9]) {
    double wsum = 0.0, acc[3] = {0.0, 0.0, 0.0}, A[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gW[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
    for (int b = 0; b < fr.nb; b++) {
        double R[9], pos[3];
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = (double)fr.sR[b * 9 + i];
#pragma unroll
        for (int c = 0; c < 3; c++)
            pos[c] = ((R[c * 3] * p[0] + R[c * 3 + 1] * p[1]) + R[c * 3 + 2] * p[2]) + (double)fr.sT[b * 3 + c];
        const PoseTap t = pose_tap(pos, fr.bmin, fr.bscale, fr.G);
        if (!t.ok) continue;
        double v[8];
        pose_corners(fr.vol + (size_t)b * fr.vsz, fr.G, t, v);
        const double w = pose_weight(t, v);
        wsum = wsum + w;
#pragma unroll
        for (int c = 0; c < 3; c++) acc[c] = acc[c] + w * pos[c];
        if (kJac) {
            double dx = 0.0, dy = 0.0, dz = 0.0;
#pragma unroll
            for (int i = 0; i < 2; i++) {
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const double wxj = j ? t.w1[0] : t.w0[0], wyj = j ? t.w1[1] : t.w0[1];
                    const double wyi = i ? t.w1[1] : t.w0[1], wzi = i ? t.w1[2] : t.w0[2];
                    dx = dx + (v[i * 4 + j * 2 + 1] - v[i * 4 + j * 2]) * (wyj * wzi);      // (z, y) = (i, j)
                    dy = dy + (v[i * 4 + 2 + j] - v[i * 4 + j]) * (wxj * wzi);              // (z, x) = (i, j)
                    dz = dz + (v[4 + i * 2 + j] - v[i * 2 + j]) * (wxj * wyi);              // (y, x) = (i, j)
                }
            }
            const double gp0 = dx * fr.k[0], gp1 = dy * fr.k[1], gp2 = dz * fr.k[2];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double gw = (gp0 * R[j] + gp1 * R[3 + j]) + gp2 * R[6 + j];
                gW[j] = gW[j] + gw;
#pragma unroll
                for (int a = 0; a < 3; a++) A[a * 3 + j] = A[a * 3 + j] + (pos[a] * gw + w * R[a * 3 + j]);
            }
        }
    }
    const bool clamped = wsum < kPoseClamp;
    const double den = clamped ? kPoseClamp : wsum;
#pragma unroll
    for (int c = 0; c < 3; c++) F[c] = acc[c] / den;
    wsum_out = wsum;
    if (kJac) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
#pragma unroll
            for (int j = 0; j < 3; j++) J[a * 3 + j] = (clamped ? A[a * 3 + j] : A[a * 3 + j] - F[a] * gW[j]) / den;
        }
    }
}

// The next bone after (c_prev, b_prev) in the order (descending canonical weight, ascending index) among those with a
// positive weight; -1 when there is none.
__device__ __forceinline__ int pose_next_candidate(const PoseFrame &fr, const PoseTap &at_xc, double &c_prev, int b_prev) {
    double best_c = 0.0;
    int best_b = -1;
    if (at_xc.ok) {
#pragma unroll 1
        for (int b = 0; b < fr.nb; b++) {
            double v[8];
            pose_corners(fr.vol + (size_t)b * fr.vsz, fr.G, at_xc, v);
            const double c = pose_weight(at_xc, v);
            if (c > best_c && (c < c_prev || (c == c_prev && b > b_prev))) best_c = c, best_b = b;
        }
    }
    if (best_b >= 0) c_prev = best_c;
    return best_b;
}

__global__ __launch_bounds__(kPoseThreads) void mesh_pose_kernel(
    const float *__restrict__ x_c, int64_t V, const float *__restrict__ Rs, const float *__restrict__ Ts,
    const float *__restrict__ vol, int nb, int G, PoseParams prm, int candidates, int max_iter, double tol,
    float *__restrict__ p_out, uint8_t *__restrict__ flag_out, uint8_t *__restrict__ iters_out, float *__restrict__ resid_out) {
    __shared__ float sR[kPoseMaxBones * 9];
    __shared__ float sT[kPoseMaxBones * 3];
    for (int i = threadIdx.x; i < nb * 9; i += blockDim.x) sR[i] = Rs[i];
    for (int i = threadIdx.x; i < nb * 3; i += blockDim.x) sT[i] = Ts[i];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kPoseThreads + threadIdx.x;
    if (i >= V) return;

    PoseFrame fr;
    fr.sR = sR, fr.sT = sT, fr.vol = vol, fr.nb = nb, fr.G = G, fr.vsz = (size_t)G * G * G;
    double xc[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        fr.bmin[c] = (double)prm.bmin[c];
        fr.bscale[c] = (double)prm.bscale[c];
        fr.k[c] = (fr.bscale[c] * (double)(G - 1)) / 2.0;
        xc[c] = (double)x_c[i * 3 + c];
    }
    const PoseTap at_xc = pose_tap(xc, fr.bmin, fr.bscale, G);

    double pb[3] = {xc[0], xc[1], xc[2]}, best = __builtin_inf();
    double F[3], J[9], wsum;
    int steps = 0, flag = 2, b_prev = -1;
    double c_prev = __builtin_inf();
#pragma unroll 1
    for (int cand = 0; cand < candidates && flag != 0; cand++) {
        const int b = pose_next_candidate(fr, at_xc, c_prev, b_prev);
        if (b < 0) break;
        b_prev = b;
        flag = 1;
        double p[3];
        {
            const double d0 = xc[0] - (double)sT[b * 3], d1 = xc[1] - (double)sT[b * 3 + 1], d2 = xc[2] - (double)sT[b * 3 + 2];
#pragma unroll
            for (int j = 0; j < 3; j++)
                p[j] = ((double)sR[b * 9 + j] * d0 + (double)sR[b * 9 + 3 + j] * d1) + (double)sR[b * 9 + 6 + j] * d2;
        }
        pose_eval<true>(fr, p, F, wsum, J);
#pragma unroll 1
        for (int it = 0;; it++) {
            const double rn = pose_norm(F, xc);
            if (rn < best) best = rn, pb[0] = p[0], pb[1] = p[1], pb[2] = p[2];
            if (rn <= tol && wsum >= kPoseClamp) {
                flag = 0, best = rn, pb[0] = p[0], pb[1] = p[1], pb[2] = p[2];
                break;
            }
            if (it == max_iter) break;
            // J delta = -r by Cramer's rule
            const double n0 = -(F[0] - xc[0]), n1 = -(F[1] - xc[1]), n2 = -(F[2] - xc[2]);
            const double m_ei = J[4] * J[8] - J[5] * J[7], m_di = J[3] * J[8] - J[5] * J[6], m_dh = J[3] * J[7] - J[4] * J[6];
            const double det = (J[0] * m_ei - J[1] * m_di) + J[2] * m_dh;
            if (det == 0.0 || !(fabs(det) <= 1.7976931348623157e308)) break;
            const double q1 = n1 * J[8] - J[5] * n2, q2 = n1 * J[7] - J[4] * n2, q3 = J[3] * n2 - n1 * J[6];
            double delta[3];
            delta[0] = ((n0 * m_ei - J[1] * q1) + J[2] * q2) / det;
            delta[1] = ((J[0] * q1 - n0 * m_di) + J[2] * q3) / det;
            delta[2] = ((J[0] * (J[4] * n2 - n1 * J[7]) - J[1] * q3) + n0 * m_dh) / det;
            steps++;
            double step = 1.0;
#pragma unroll 1
            for (int h = 0;; h++) {
                double q[3];
#pragma unroll
                for (int c = 0; c < 3; c++) q[c] = p[c] + step * delta[c];
                pose_eval<true>(fr, q, F, wsum, J);      // (the old F and J are spent: delta holds what the retries need)
                if (pose_norm(F, xc) < rn || h == 5) {
                    p[0] = q[0], p[1] = q[1], p[2] = q[2];
                    break;
                }
                step = step * 0.5;
            }
        }
    }
    if (flag == 2) {
        pose_eval<false>(fr, xc, F, wsum, J);
        best = pose_norm(F, xc);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) p_out[i * 3 + c] = (float)pb[c];
    flag_out[i] = (uint8_t)flag;
    iters_out[i] = (uint8_t)(steps > 255 ? 255 : steps);
    resid_out[i] = (float)best;
}

}  // namespace occ

OCC_API int occnerf_mesh_pose(const float *x_c, int64_t V, const float *Rs, const float *Ts, const float *vol, int32_t nb,
                              int32_t G, const float *h_bbox_min, const float *h_bbox_scale, int32_t candidates,
                              int32_t max_iter, double tol, float *p_out, uint8_t *flag, uint8_t *iters, float *resid,
                              void *stream) {
    using namespace occ;
    OCC_REQUIRE(Rs && Ts && vol && h_bbox_min && h_bbox_scale, "mesh_pose: null argument");
    OCC_REQUIRE(nb >= 1 && nb <= kPoseMaxBones, "mesh_pose: nb=%d outside 1..%d", nb, kPoseMaxBones);
    OCC_REQUIRE(G >= 2 && G <= 1024, "mesh_pose: G=%d outside 2..1024", G);
    OCC_REQUIRE(candidates >= 1 && candidates <= 8, "mesh_pose: candidates=%d outside 1..8", candidates);
    OCC_REQUIRE(max_iter >= 1 && max_iter <= 255, "mesh_pose: max_iter=%d outside 1..255", max_iter);
    OCC_REQUIRE(tol >= 0.0 && tol <= 1.7976931348623157e308, "mesh_pose: tol=%g must be a finite number >= 0", tol);
    OCC_REQUIRE(V >= 0 && V < (1ll << 31) * kPoseThreads, "mesh_pose: V=%lld out of range", (long long)V);
    if (V == 0) return 0;
    OCC_REQUIRE(x_c && p_out && flag && iters && resid, "mesh_pose: null x_c / output with V=%lld", (long long)V);
    PoseParams prm;
    for (int c = 0; c < 3; c++) {
        prm.bmin[c] = h_bbox_min[c];
        prm.bscale[c] = h_bbox_scale[c];
    }
    hipLaunchKernelGGL(mesh_pose_kernel, dim3((unsigned)((V + kPoseThreads - 1) / kPoseThreads)), dim3(kPoseThreads), 0,
                       as_stream(stream), x_c, V, Rs, Ts, vol, nb, G, prm, candidates, max_iter, tol, p_out, flag, iters, resid);
    return check_launch("mesh_pose");
}
