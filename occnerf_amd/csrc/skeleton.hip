// The driving skeleton of an animate frame, drawn from the frame's own camera (no counterpart in the
// reference, which has no entry point for a novel motion): 23 bones as thick segments and 24 joints as discs over the
// background colour.  One launch, one thread per pixel, no atomics: every workgroup projects the 24 joints itself (float64,
// one rounding per operator -- the tree is built with -ffp-contract=off -- division correctly rounded), stages the 47
// primitives in LDS once, and every thread then walks them in index order.  The bytes are a pure function of the inputs,
// bit-identical to tests/skeleton_restatement.py.
//
// Bound: the walk, 47 primitives x about 20 float64 operations per pixel from LDS broadcasts (every lane reads the same
// address: no bank conflict); the image is written once, 3 bytes per pixel.  The count record needs no second launch: slot 0
// is the number of dropped joints (workgroup 0 writes it), slot 1 + b the pixels workgroup b covered; the host adds them.
#include "batch_common.h"

namespace occ {

constexpr int kSkelJoints = 24;
constexpr int kSkelBones = kSkelJoints - 1;
constexpr int kSkelPrims = kSkelBones + kSkelJoints;

// SMPL's kinematic tree: the parent of joint c (synth.SMPL_PARENT); bone b joins joint b + 1 and its parent.
__constant__ int8_t kSkelParent[kSkelJoints] = {-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21};

struct SkeletonParams {
    float joints[kSkelJoints * 3];     // body space, the space of the rays
    double fx, fy, cx, cy;             // K without skew
    double R[9], t[3];                 // E[:3,:3], E[:3,3]
    double bone_px;                    // half-width of a bone; a joint's disc has 1.5 x that
    uint8_t palette[kSkelJoints * 3];  // the colour of bone b is that of its child joint b + 1
    uint8_t bg[3];
};

__device__ __forceinline__ bool finite_f64(double x) {
    return (__double2hiint(x) & 0x7ff00000) != 0x7ff00000;
}

__global__ __launch_bounds__(kBatchThreads) void skeleton_panel_kernel(SkeletonParams prm, int32_t H, int32_t W,
                                                                       uint8_t *__restrict__ img, int32_t *__restrict__ record) {
    __shared__ double ju[kSkelJoints], jv[kSkelJoints], jz[kSkelJoints];
    __shared__ int jok[kSkelJoints];
    // a primitive: the segment a + s ab (s in 0..1) of squared radius r2 and depth key `key`; l2 = |ab|^2, 0 for a disc
    __shared__ double pax[kSkelPrims], pay[kSkelPrims], pabx[kSkelPrims], paby[kSkelPrims], pl2[kSkelPrims], pr2[kSkelPrims],
        pkey[kSkelPrims];
    __shared__ int pok[kSkelPrims], pcol[kSkelPrims];          // pcol: the colour, r | g << 8 | b << 16
    __shared__ int red[kBatchWaves];
    const int tid = threadIdx.x;
    if (tid < kSkelJoints) {
        const double x = (double)prm.joints[tid * 3], y = (double)prm.joints[tid * 3 + 1], z = (double)prm.joints[tid * 3 + 2];
        const double c0 = ((prm.R[0] * x + prm.R[1] * y) + prm.R[2] * z) + prm.t[0];
        const double c1 = ((prm.R[3] * x + prm.R[4] * y) + prm.R[5] * z) + prm.t[1];
        const double c2 = ((prm.R[6] * x + prm.R[7] * y) + prm.R[8] * z) + prm.t[2];
        const double u = __ddiv_rn(prm.fx * c0, c2) + prm.cx;
        const double v = __ddiv_rn(prm.fy * c1, c2) + prm.cy;
        const bool ok = finite_f64(c0) && finite_f64(c1) && finite_f64(c2) && c2 > 0.0 && finite_f64(u) && finite_f64(v);
        ju[tid] = u;
        jv[tid] = v;
        jz[tid] = c2;
        jok[tid] = ok ? 1 : 0;
    }
    __syncthreads();
    if (tid < kSkelPrims) {
        const double r = tid < kSkelBones ? prm.bone_px : 1.5 * prm.bone_px;
        const int a = tid < kSkelBones ? tid + 1 : tid - kSkelBones;      // the child joint, or the disc's own
        const int b = tid < kSkelBones ? kSkelParent[a] : a;
        const double abx = ju[b] - ju[a], aby = jv[b] - jv[a];
        pax[tid] = ju[a];
        pay[tid] = jv[a];
        pabx[tid] = abx;
        paby[tid] = aby;
        pl2[tid] = abx * abx + aby * aby;
        pr2[tid] = r * r;
        pkey[tid] = tid < kSkelBones ? (jz[a] + jz[b]) * 0.5 : jz[a];
        pok[tid] = jok[a] & jok[b];
        pcol[tid] = prm.palette[a * 3] | (prm.palette[a * 3 + 1] << 8) | (prm.palette[a * 3 + 2] << 16);
    }
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * kBatchThreads + tid, n = (int64_t)H * W;
    int best = -1;
    if (p < n) {
        const int32_t i = (int32_t)(p / W), j = (int32_t)(p - (int64_t)i * W);
        const double px = (double)j, py = (double)i;      // the sample of pixel (i, j): where the renderer's ray leaves the camera
        double best_key = 0.0;
        for (int q = 0; q < kSkelPrims; q++) {
            if (!pok[q]) continue;
            const double dx = px - pax[q], dy = py - pay[q];
            double ex = dx, ey = dy;
            if (pl2[q] != 0.0) {
                double s = __ddiv_rn(dx * pabx[q] + dy * paby[q], pl2[q]);
                s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
                ex = px - (pax[q] + s * pabx[q]);
                ey = py - (pay[q] + s * paby[q]);
            }
            const double d2 = ex * ex + ey * ey;
            if (d2 <= pr2[q] && (best < 0 || pkey[q] <= best_key)) {      // the nearer one; at equal keys the higher index
                best = q;
                best_key = pkey[q];
            }
        }
        const int c = best >= 0 ? pcol[best] : (prm.bg[0] | (prm.bg[1] << 8) | (prm.bg[2] << 16));
        img[p * 3] = (uint8_t)c;
        img[p * 3 + 1] = (uint8_t)(c >> 8);
        img[p * 3 + 2] = (uint8_t)(c >> 16);
    }
    const int covered = block_sum(best >= 0 ? 1 : 0, red);
    if (tid == 0) {
        record[1 + blockIdx.x] = covered;
        if (blockIdx.x == 0) {
            int dropped = 0;
            for (int k = 0; k < kSkelJoints; k++) dropped += 1 - jok[k];
            record[0] = dropped;
        }
    }
}

constexpr int64_t kSkelMaxPixels = (int64_t)1 << 31;

}  // namespace occ

OCC_API int32_t occnerf_skeleton_panel_blocks(int32_t height, int32_t width) {
    if (height < 1 || width < 1 || (int64_t)height * width >= occ::kSkelMaxPixels) return 0;
    return (int32_t)(((int64_t)height * width + occ::kBatchThreads - 1) / occ::kBatchThreads);
}

OCC_API int occnerf_skeleton_panel(const float *h_joints, const double *h_K, const double *h_E, double bone_px,
                                   const uint8_t *h_palette, const uint8_t *h_bgcolor, int32_t height, int32_t width,
                                   uint8_t *img, int32_t *record, void *stream) {
    using namespace occ;
    OCC_REQUIRE(height >= 1 && width >= 1 && (int64_t)height * width < kSkelMaxPixels, "skeleton_panel: bad sizes");
    OCC_REQUIRE(h_joints && h_K && h_E && h_palette && h_bgcolor && img && record, "skeleton_panel: null argument");
    OCC_REQUIRE(h_K[1] == 0.0, "skeleton_panel: skew K[0,1] = %g is not built", h_K[1]);
    OCC_REQUIRE(bone_px >= 0.0 && bone_px <= 1.0e6, "skeleton_panel: bone_px = %g outside 0..1e6", bone_px);
    SkeletonParams prm;
    for (int k = 0; k < kSkelJoints * 3; k++) {
        prm.joints[k] = h_joints[k];
        prm.palette[k] = h_palette[k];
    }
    prm.fx = h_K[0], prm.fy = h_K[4], prm.cx = h_K[2], prm.cy = h_K[5];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) prm.R[r * 3 + c] = h_E[r * 4 + c];
        prm.t[r] = h_E[r * 4 + 3];
    }
    prm.bone_px = bone_px;
    for (int c = 0; c < 3; c++) prm.bg[c] = h_bgcolor[c];
    const int64_t n = (int64_t)height * width;
    hipLaunchKernelGGL(skeleton_panel_kernel, dim3((unsigned)((n + kBatchThreads - 1) / kBatchThreads)), dim3(kBatchThreads), 0,
                       as_stream(stream), prm, height, width, img, record);
    return check_launch("skeleton_panel");
}
