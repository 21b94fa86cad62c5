// The image step of the trainer's progress dump (trainer.py:346-383 of the reference): per held-out frame the reference
// scatters the rays' colours into an H x W float image on the host, quantises it and the truth (to_8b_image), joins the two
// panels side by side, tests the rendered panel with np.allclose(rendered, cfg.bgcolor, atol=3.) and, after the last frame,
// tiles the panels four to a row (image_util.py:38-50).  Here one launch per frame writes both panels straight into their
// tile of the mosaic on the device and counts the rendered bytes that are off the background; nothing crosses PCIe per frame.
//
// Kernel 1: one thread per pixel, as assemble_image_kernel (image.hip): a binary search in the ascending ray_index[R] finds
// the pixel's ray or learns that it has none, to_8b (batch_common.h) quantises, and the pixel's three rendered bytes go to
// mosaic row ty*H + y, column tx*2W + x, the three bytes of truth_u8 to column tx*2W + W + x.  Consecutive lanes write
// consecutive bytes of one mosaic row.  The off-background test is np.allclose's on a uint8 array against a float64 one:
// |v - b| <= 3 + 1e-5 |b| in fp64, one rounding per operator.  The workgroup's count of failing bytes goes to partial[block].
// Kernel 2: one workgroup sums the partials into off_bg[frame].  Integers: every order gives the same value; no atomics.
// Bound: HBM streaming, 12 B per ray and 3 B per pixel in, 6 B per pixel out.
#include "batch_common.h"

namespace occ {

struct ProgressParams {
    float bg01[3];        // float32(cfg.bgcolor / 255): the colour of a pixel without a ray
    double bg255[3];      // cfg.bgcolor as given: what allclose compares the rendered bytes with
    double tol[3];        // atol + rtol * |bg255|
};

__global__ __launch_bounds__(kBatchThreads) void progress_tile_kernel(
    const float *__restrict__ rgb, const int64_t *__restrict__ ray_index, int64_t R, int H, int W, ProgressParams prm,
    const uint8_t *__restrict__ truth, uint8_t *__restrict__ mosaic, int64_t row_bytes, int64_t tile_byte0,
    int32_t *__restrict__ partial) {
    __shared__ int red[kBatchWaves];
    const int64_t n_pixels = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int off = 0;
    if (p < n_pixels) {
        int64_t lo = 0, hi = R;                             // first ray with ray_index >= p
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (ray_index[mid] < p) lo = mid + 1;
            else hi = mid;
        }
        const bool hit = lo < R && ray_index[lo] == p;
        const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
        uint8_t *dst = mosaic + tile_byte0 + y * row_bytes + (int64_t)x * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const uint8_t q = to_8b(hit ? rgb[lo * 3 + c] : prm.bg01[c]);
            dst[c] = q;
            dst[(int64_t)W * 3 + c] = truth[p * 3 + c];
            const double d = fabs(__dsub_rn((double)q, prm.bg255[c]));
            off += d > prm.tol[c] ? 1 : 0;                  // not allclose: |a - b| <= atol + rtol |b| fails
        }
    }
    const int total = block_sum(off, red);                  // every thread of the workgroup reaches it
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBatchThreads) void progress_count_kernel(const int32_t *__restrict__ partial, int n,
                                                                       int32_t *__restrict__ off_bg) {
    __shared__ int red[kBatchWaves];
    int s = 0;
    for (int i = threadIdx.x; i < n; i += kBatchThreads) s += partial[i];
    const int total = block_sum(s, red);
    if (threadIdx.x == 0) *off_bg = total;
}

}  // namespace occ

OCC_API int32_t occnerf_progress_tile_blocks(int32_t height, int32_t width) {
    if (height <= 0 || width <= 0 || (int64_t)height * width >= ((int64_t)1 << 28)) return -1;
    return (int32_t)(((int64_t)height * width + occ::kBatchThreads - 1) / occ::kBatchThreads);
}

OCC_API int occnerf_progress_tile(const float *rgb, const int64_t *ray_index, int64_t R, int32_t height, int32_t width,
                                  const float *h_bgcolor01, const double *h_bgcolor255, const uint8_t *truth_u8,
                                  uint8_t *mosaic, int32_t mosaic_rows, int32_t mosaic_cols, int32_t tile_x, int32_t tile_y,
                                  int32_t *partial, int32_t *off_bg, void *stream) {
    using namespace occ;
    const int32_t blocks = occnerf_progress_tile_blocks(height, width);
    OCC_REQUIRE(blocks > 0 && R >= 0 && R <= (int64_t)height * width, "progress_tile: bad sizes (H * W must be below 2^28)");
    OCC_REQUIRE(h_bgcolor01 && h_bgcolor255 && truth_u8 && mosaic && partial && off_bg && (R == 0 || (rgb && ray_index)),
                "progress_tile: null argument");
    OCC_REQUIRE(tile_x >= 0 && tile_y >= 0 && mosaic_rows > 0 && mosaic_cols > 0 &&
                    ((int64_t)tile_x + 1) * 2 * width <= mosaic_cols && ((int64_t)tile_y + 1) * height <= mosaic_rows,
                "progress_tile: tile (%d, %d) of %d x %d panels does not fit a mosaic of %d x %d pixels", tile_x, tile_y,
                2 * width, height, mosaic_cols, mosaic_rows);
    ProgressParams prm;
    for (int c = 0; c < 3; c++) {
        prm.bg01[c] = h_bgcolor01[c];
        prm.bg255[c] = h_bgcolor255[c];
        const volatile double rel = 1e-5 * fabs(h_bgcolor255[c]);      // two roundings, as numpy's atol + rtol * abs(b)
        prm.tol[c] = 3.0 + rel;
    }
    const int64_t row_bytes = (int64_t)mosaic_cols * 3;
    const int64_t tile_byte0 = (int64_t)tile_y * height * row_bytes + (int64_t)tile_x * 2 * width * 3;
    hipLaunchKernelGGL(progress_tile_kernel, dim3((unsigned)blocks), dim3(kBatchThreads), 0, as_stream(stream), rgb, ray_index,
                       R, (int)height, (int)width, prm, truth_u8, mosaic, row_bytes, tile_byte0, partial);
    hipLaunchKernelGGL(progress_count_kernel, dim3(1), dim3(kBatchThreads), 0, as_stream(stream), partial, (int)blocks, off_bg);
    return check_launch("progress_tile");
}
