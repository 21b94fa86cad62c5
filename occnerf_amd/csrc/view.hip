// The rays of a camera that has no photograph (freeview / backview / allview / tpose on a prepared dataset, views.py): the
// rays-only form of frame.hip's row gather.  occnerf_gen_rays has written the ray of every pixel and the box mask,
// occnerf_whole_frame_count the hits above every image row; one workgroup per image row then walks the row in chunks of 256
// pixels and compacts the hits in order (ballot + mbcnt prefix, one LDS scan across the four waves) starting at
// row_start[row], so the rows come out in row-major pixel order, np.nonzero's.  32 bytes read and 36 written per hit; no image
// is read and no per-pixel map is written.  No atomics, no host wait; every output is a pure function of the inputs.
#include "batch_common.h"

namespace occ {

__global__ __launch_bounds__(kBatchThreads) void view_gather_kernel(const float *__restrict__ rays8,
                                                                   const uint8_t *__restrict__ box, int W,
                                                                   const int32_t *__restrict__ row_start, int R,
                                                                   int64_t *__restrict__ ray_index, float *__restrict__ rays,
                                                                   float *__restrict__ near, float *__restrict__ far) {
    __shared__ int red[kBatchWaves];
    const int y = blockIdx.x, t = threadIdx.x;
    int base = row_start[y];
    for (int x0 = 0; x0 < W; x0 += kBatchThreads) {
        const int x = x0 + t;
        const size_t p = (size_t)y * W + (x < W ? x : 0);
        const bool hit = x < W && box[p] != 0;
        int chunk;
        const int row = base + chunk_rank(hit, red, chunk);
        base += chunk;
        if (hit && row < R) {                          // row < R: a caller's R below the scan's total cannot write past the end
            ray_index[row] = (int64_t)p;
            store_ray_row(rays8 + p * 8, row, R, rays, near, far);
        }
    }
}

}  // namespace occ

OCC_API int occnerf_view_frame_gather(const float *rays8, const uint8_t *box_mask, int32_t H, int32_t W,
                                      const int32_t *row_start, int32_t R, int64_t *ray_index, float *rays, float *near,
                                      float *far, void *stream) {
    using namespace occ;
    OCC_REQUIRE(rays8 && box_mask && row_start, "view_frame_gather: null argument");
    OCC_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < (1ll << 28), "view_frame_gather: bad image size %d x %d", H, W);
    OCC_REQUIRE(R >= 0 && (int64_t)R <= (int64_t)H * W, "view_frame_gather: R=%d outside [0, %lld]", R, (long long)H * W);
    OCC_REQUIRE(R == 0 || (ray_index && rays && near && far), "view_frame_gather: null ray output with R=%d", R);
    hipLaunchKernelGGL(view_gather_kernel, dim3(H), dim3(kBatchThreads), 0, as_stream(stream), rays8, box_mask, W, row_start,
                       R, ray_index, rays, near, far);
    return check_launch("view_frame_gather");
}
