// A whole frame of a prepared dataset, built on the device: what PreparedDataset.whole_frame() (the reference's
// `ray_shoot_mode 'image'` dict, core/data/occnerf/train.py:353-537) returns for the frame, plus the per-pixel maps
// eval.py's metrics take.  The frame's image and mask stay resident as uint8; occnerf_gen_rays has written the ray of
// every pixel and the box mask.  Two calls, because the row count R sets the output shapes and the offset of the direction
// half of rays[2,R,3]:
//   occnerf_whole_frame_count    one workgroup per image row counts the row's box hits (wave64 ballots and popcounts); one
//                                workgroup then scans the H counts in place, 256 rows at a time: row_start[row] = hits of
//                                the rows above, row_start[H] = R;
//   occnerf_whole_frame_gather   one workgroup per image row walks the row in chunks of 256 pixels: ordered compaction of
//                                the hits (ballot + mbcnt prefix, one LDS scan across the four waves) starting at
//                                row_start[row], so the rows come out in row-major pixel order, np.nonzero's.  Every
//                                pixel writes its map entries, every hit its ray row.
// No atomics, no host wait inside a call; every output is a pure function of the inputs.  The blend and the 8-bit
// quantisation are batch_common.h's, the ones the patch batch and the image assembly use.
#include "batch_common.h"

namespace occ {

__global__ __launch_bounds__(kBatchThreads) void frame_count_kernel(const uint8_t *__restrict__ box, int W,
                                                                   int32_t *__restrict__ row_start) {
    __shared__ int red[kBatchWaves];
    const int row = blockIdx.x;
    int n = 0;
    for (int x0 = 0; x0 < W; x0 += kBatchThreads) {
        const int x = x0 + threadIdx.x;
        const bool hit = x < W && box[(size_t)row * W + x] != 0;
        n += __popcll(__ballot(hit));                  // wave-uniform
    }
    const int total = block_sum((threadIdx.x & (kWave - 1)) == 0 ? n : 0, red);
    if (threadIdx.x == 0) row_start[row] = total;
}

// row_start[0..H) holds the row counts; in place -> their exclusive prefix, row_start[H] = the total.  One workgroup.
__global__ __launch_bounds__(kBatchThreads) void frame_scan_kernel(int H, int32_t *__restrict__ row_start) {
    __shared__ int red[kBatchWaves];
    int carry = 0;
    for (int r0 = 0; r0 < H; r0 += kBatchThreads) {
        const int r = r0 + threadIdx.x;
        const int v = r < H ? row_start[r] : 0;
        int total;
        const int excl = block_excl_scan(v, red, total);
        if (r < H) row_start[r] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) row_start[H] = carry;
}

struct FrameOut {
    int64_t *ray_index;
    float *rays, *near, *far, *target_rgbs;
    double *ray_alpha;
    uint8_t *truth_u8;
    float *gt_vis, *gt_alpha;
};

// Pixels: where the frame's pixels are read from, PixelsU8 or PixelsF64 (batch_common.h)
template <class Pixels>
__global__ __launch_bounds__(kBatchThreads) void frame_gather_kernel(const Pixels px, const float *__restrict__ rays8,
                                                                    const uint8_t *__restrict__ box, int W, double bg0,
                                                                    double bg1, double bg2,
                                                                    const int32_t *__restrict__ row_start, int R,
                                                                    FrameOut out) {
    __shared__ int red[kBatchWaves];
    const int y = blockIdx.x, t = threadIdx.x;
    const double bg[3] = {bg0, bg1, bg2};
    int base = row_start[y];
    for (int x0 = 0; x0 < W; x0 += kBatchThreads) {
        const int x = x0 + t;
        const bool live = x < W;
        const size_t p = (size_t)y * W + (live ? x : 0);
        const bool hit = live && box[p] != 0;
        int chunk;
        const int row = base + chunk_rank(hit, red, chunk);
        base += chunk;
        if (!live) continue;
        const float a0 = px.alpha0(p);
        out.gt_alpha[p] = a0;
        out.gt_vis[p] = hit ? a0 : 0.0f;
        float rgb[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            // inside the box the truth image shows the blended photograph, outside float32(bgcolor / 255) (unpack_to_image)
            rgb[c] = hit ? px.target(p, c, bg[c]) : (float)__ddiv_rn(bg[c], 255.0);
            out.truth_u8[p * 3 + c] = to_8b(rgb[c]);
        }
        if (hit && row < R) {                          // row < R: a caller's R below the scan's total cannot write past the end
            out.ray_index[row] = (int64_t)p;
            store_ray_row(rays8 + p * 8, row, R, out.rays, out.near, out.far);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                out.target_rgbs[(int64_t)row * 3 + c] = rgb[c];
                out.ray_alpha[(int64_t)row * 3 + c] = px.alpha(p, c);
            }
        }
    }
}

}  // namespace occ

OCC_API int occnerf_whole_frame_count(const uint8_t *box_mask, int32_t H, int32_t W, int32_t *row_start, void *stream) {
    using namespace occ;
    OCC_REQUIRE(box_mask && row_start, "whole_frame_count: null argument");
    OCC_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < (1ll << 28), "whole_frame_count: bad image size %d x %d", H, W);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(frame_count_kernel, dim3(H), dim3(kBatchThreads), 0, st, box_mask, W, row_start);
    hipLaunchKernelGGL(frame_scan_kernel, dim3(1), dim3(kBatchThreads), 0, st, H, row_start);
    return check_launch("whole_frame_count");
}

namespace occ {

// The gather from either pixel source; `first` and `second` are its two pointers, checked with the rest.
template <class Pixels>
static int whole_frame_gather_from(const Pixels px, const void *first, const void *second, const float *rays8,
                                   const uint8_t *box_mask, int32_t H, int32_t W, const float *h_bgcolor,
                                   const int32_t *row_start, int32_t R, int64_t *ray_index, float *rays, float *near,
                                   float *far, float *target_rgbs, double *ray_alpha, uint8_t *truth_u8, float *gt_vis,
                                   float *gt_alpha, void *stream) {
    OCC_REQUIRE(first && second && rays8 && box_mask && h_bgcolor && row_start && truth_u8 && gt_vis && gt_alpha,
                "whole_frame_gather: null argument");
    OCC_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < (1ll << 28), "whole_frame_gather: bad image size %d x %d", H, W);
    OCC_REQUIRE(R >= 0 && (int64_t)R <= (int64_t)H * W, "whole_frame_gather: R=%d outside [0, %lld]", R, (long long)H * W);
    OCC_REQUIRE(R == 0 || (ray_index && rays && near && far && target_rgbs && ray_alpha),
                "whole_frame_gather: null ray output with R=%d", R);
    FrameOut out{ray_index, rays, near, far, target_rgbs, ray_alpha, truth_u8, gt_vis, gt_alpha};
    hipLaunchKernelGGL(frame_gather_kernel<Pixels>, dim3(H), dim3(kBatchThreads), 0, as_stream(stream), px, rays8, box_mask,
                       W, (double)h_bgcolor[0], (double)h_bgcolor[1], (double)h_bgcolor[2], row_start, R, out);
    return check_launch("whole_frame_gather");
}

}  // namespace occ

OCC_API int occnerf_whole_frame_gather(const uint8_t *image, const uint8_t *alpha, const float *rays8, const uint8_t *box_mask,
                                       int32_t H, int32_t W, const float *h_bgcolor, const int32_t *row_start, int32_t R,
                                       int64_t *ray_index, float *rays, float *near, float *far, float *target_rgbs,
                                       double *ray_alpha, uint8_t *truth_u8, float *gt_vis, float *gt_alpha, void *stream) {
    return occ::whole_frame_gather_from(occ::PixelsU8{image, alpha}, image, alpha, rays8, box_mask, H, W, h_bgcolor, row_start,
                                        R, ray_index, rays, near, far, target_rgbs, ray_alpha, truth_u8, gt_vis, gt_alpha,
                                        stream);
}

OCC_API int occnerf_whole_frame_gather_f64(const double *img64, const double *alpha64, const float *rays8,
                                           const uint8_t *box_mask, int32_t H, int32_t W, const float *h_bgcolor,
                                           const int32_t *row_start, int32_t R, int64_t *ray_index, float *rays, float *near,
                                           float *far, float *target_rgbs, double *ray_alpha, uint8_t *truth_u8,
                                           float *gt_vis, float *gt_alpha, void *stream) {
    return occ::whole_frame_gather_from(occ::PixelsF64{img64, alpha64}, img64, alpha64, rays8, box_mask, H, W, h_bgcolor,
                                        row_start, R, ray_index, rays, near, far, target_rgbs, ray_alpha, truth_u8, gt_vis,
                                        gt_alpha, stream);
}
