// Resizing a prepared frame to the training size (the reference's two cv2.resize lines, core/data/occnerf/train.py:306-314):
// occnerf_amd/resize.py's resize_blend on the device, bit for bit.  The float64 blend of the
// full-size photograph over the background, (m / 255.) * I + (1.0 - m / 255.) * bg, is resized with the eight-tap Lanczos
// filter and m / 255. with the bilinear one; both passes are left-to-right float64 sums of source * weight that start at
// 0.0, the horizontal pass first.  The tap offsets and weights of both axes are tables the host builds once per dataset
// (there is no sin or cos here); the operators are spelt __d*_rn as batch_common.h's blend is, the tree is built with
// -ffp-contract=off.
//
// One workgroup of 256 threads makes a tile of kTileW output columns by `tile_h` <= kTileH output rows:
//   0. m -> m / 255. (256 divisions per workgroup, not one per tap) and (c, m) -> (1.0 - m / 255.) * bg[c] into LDS;
//   1. the horizontal sums of the tile's columns over the source rows the tile's vertical taps reach -- rows
//      y_lo .. y_lo + span - 1, span <= kRows -- into LDS, once: a thread owns one column (its taps stay in registers) and
//      walks the rows, six channels from one set of offsets;
//   2. the vertical sums from LDS, one output pixel per thread, six float64 stores.
// At s = 1/2 a tile of 8 rows reads 22 source rows, so a horizontal sum is computed 1.4 times instead of the 8 (Lanczos)
// and 2 (bilinear) times a per-pixel kernel would.  The LDS rows are [row][channel][column]: the 32 lanes of a ds_read_b64
// group read 256 contiguous bytes, no bank is hit twice.  No atomics, no host wait, plain vector stores.
//
// The entry checks the HOST copies of the offset tables (every offset inside the image, the row span of a tile within
// kRows) before it launches; the kernel clamps what it reads from the device copies all the same, so a device table that
// differs from its host copy gives wrong pixels, never an access outside the image or the tile.
#include "batch_common.h"

namespace occ {

constexpr int kTileW = 32, kTileH = kBatchThreads / kTileW;      // 32 x 8 output pixels
constexpr int kRows = 24;                                         // source rows of a tile held in LDS (2 * 7 + 8 = 22 at 1/2)
constexpr int kLanczos = 8, kLinear = 2;

struct ResizeTables {                                             // device pointers: offsets int32, weights float32
    const int32_t *x_off_l, *y_off_l, *x_off_b, *y_off_b;         // [w,8], [h,8], [w,2], [h,2]
    const float *x_w_l, *y_w_l, *x_w_b, *y_w_b;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool kImage>
__global__ __launch_bounds__(kBatchThreads) void resize_kernel(const uint8_t *__restrict__ image,
                                                              const uint8_t *__restrict__ mask, int H, int W, int h, int w,
                                                              int tile_h, ResizeTables tb, double bg0, double bg1, double bg2,
                                                              double *__restrict__ img64, double *__restrict__ alpha64) {
    __shared__ double a_of[256];                                  // m / 255.
    __shared__ double bk_of[kImage ? 3 * 256 : 1];                // (1.0 - m / 255.) * bg[c]
    __shared__ double rows_a[kRows * 3 * kTileW];                 // horizontal bilinear sums of m / 255.
    __shared__ double rows_i[kImage ? kRows * 3 * kTileW : 1];    // horizontal Lanczos sums of the blend
    const int t = threadIdx.x;
    const int c0 = blockIdx.x * kTileW, r0 = blockIdx.y * tile_h;
    const int r1 = min(r0 + tile_h, h) - 1;                       // last output row of the tile
    {
        const double a = __ddiv_rn((double)t, 255.0);
        a_of[t] = a;
        if (kImage) {
            const double one_minus = __dsub_rn(1.0, a);
            bk_of[t] = __dmul_rn(one_minus, bg0);
            bk_of[256 + t] = __dmul_rn(one_minus, bg1);
            bk_of[512 + t] = __dmul_rn(one_minus, bg2);
        }
    }
    // the source rows of the tile: the tables ascend with the destination index and the Lanczos taps enclose the bilinear ones
    const int y_lo = clampi(tb.y_off_l[(size_t)r0 * kLanczos], 0, H - 1);
    const int span = clampi(tb.y_off_l[(size_t)r1 * kLanczos + kLanczos - 1] - y_lo + 1, 1, min(kRows, H - y_lo));
    __syncthreads();

    // 1. horizontal sums: thread -> column t % kTileW, rows t / kTileW, + kTileH, ...
    const int lx = t % kTileW, X = c0 + lx;
    if (X < w) {
        int xo_l[kLanczos], xo_b[kLinear];
        double xw_l[kLanczos], xw_b[kLinear];
#pragma unroll
        for (int k = 0; k < kLanczos; k++) {
            xo_l[k] = kImage ? clampi(tb.x_off_l[(size_t)X * kLanczos + k], 0, W - 1) * 3 : 0;
            xw_l[k] = kImage ? (double)tb.x_w_l[(size_t)X * kLanczos + k] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < kLinear; k++) {
            xo_b[k] = clampi(tb.x_off_b[(size_t)X * kLinear + k], 0, W - 1) * 3;
            xw_b[k] = (double)tb.x_w_b[(size_t)X * kLinear + k];
        }
        for (int row = t / kTileW; row < span; row += kTileH) {
            const size_t line = (size_t)(y_lo + row) * W * 3;
            double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < kLinear; k++) {
#pragma unroll
                for (int c = 0; c < 3; c++)
                    acc[c] = __dadd_rn(acc[c], __dmul_rn(a_of[mask[line + xo_b[k] + c]], xw_b[k]));
            }
#pragma unroll
            for (int c = 0; c < 3; c++) rows_a[(row * 3 + c) * kTileW + lx] = acc[c];
            if (kImage) {
                double sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
                for (int k = 0; k < kLanczos; k++) {
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const int m = mask[line + xo_l[k] + c];
                        const double fg = __dmul_rn(a_of[m], (double)image[line + xo_l[k] + c]);
                        sum[c] = __dadd_rn(sum[c], __dmul_rn(__dadd_rn(fg, bk_of[c * 256 + m]), xw_l[k]));
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; c++) rows_i[(row * 3 + c) * kTileW + lx] = sum[c];
            }
        }
    }
    __syncthreads();

    // 2. vertical sums: thread -> output pixel (r0 + t / kTileW, X)
    const int r = r0 + t / kTileW;
    if (X >= w || t / kTileW >= tile_h || r > r1) return;
    const size_t o = ((size_t)r * w + X) * 3;
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kLinear; k++) {
        const int row = clampi(tb.y_off_b[(size_t)r * kLinear + k] - y_lo, 0, span - 1);
        const double wk = (double)tb.y_w_b[(size_t)r * kLinear + k];
#pragma unroll
        for (int c = 0; c < 3; c++) acc[c] = __dadd_rn(acc[c], __dmul_rn(rows_a[(row * 3 + c) * kTileW + lx], wk));
    }
#pragma unroll
    for (int c = 0; c < 3; c++) alpha64[o + c] = acc[c];
    if (kImage) {
        double sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < kLanczos; k++) {
            const int row = clampi(tb.y_off_l[(size_t)r * kLanczos + k] - y_lo, 0, span - 1);
            const double wk = (double)tb.y_w_l[(size_t)r * kLanczos + k];
#pragma unroll
            for (int c = 0; c < 3; c++) sum[c] = __dadd_rn(sum[c], __dmul_rn(rows_i[(row * 3 + c) * kTileW + lx], wk));
        }
#pragma unroll
        for (int c = 0; c < 3; c++) img64[o + c] = sum[c];
    }
}

// Every offset of a host table inside [0, n_src); -> the first bad entry or -1.
static int64_t bad_offset(const int32_t *off, int64_t n, int32_t n_src) {
    for (int64_t i = 0; i < n; i++)
        if (off[i] < 0 || off[i] >= n_src) return i;
    return -1;
}

// The source rows a tile of `tile_h` output rows reaches, at most, from the host tables (both filters).
static int tile_span(const int32_t *y_l, const int32_t *y_b, int h, int tile_h) {
    int worst = 0;
    for (int r0 = 0; r0 < h; r0 += tile_h) {
        const int lo = y_l[(size_t)r0 * kLanczos];
        for (int r = r0; r < r0 + tile_h && r < h; r++) {
            for (int k = 0; k < kLanczos; k++) {
                const int v = y_l[(size_t)r * kLanczos + k];
                if (v < lo) return kRows + 1;                     // a tap above the tile's first one: not a table of resize.py
                worst = max(worst, v - lo + 1);
            }
            for (int k = 0; k < kLinear; k++) {
                const int v = y_b[(size_t)r * kLinear + k];
                if (v < lo) return kRows + 1;
                worst = max(worst, v - lo + 1);
            }
        }
    }
    return worst;
}

}  // namespace occ

OCC_API int occnerf_resize_frame(const uint8_t *image, const uint8_t *mask, int32_t H, int32_t W, int32_t h, int32_t w,
                                 const int32_t *x_off_lanczos, const float *x_w_lanczos, const int32_t *y_off_lanczos,
                                 const float *y_w_lanczos, const int32_t *x_off_bilinear, const float *x_w_bilinear,
                                 const int32_t *y_off_bilinear, const float *y_w_bilinear, const int32_t *h_x_off_lanczos,
                                 const int32_t *h_y_off_lanczos, const int32_t *h_x_off_bilinear,
                                 const int32_t *h_y_off_bilinear, const float *h_bgcolor, double *img64, double *alpha64,
                                 void *stream) {
    using namespace occ;
    OCC_REQUIRE(mask && alpha64, "resize_frame: null mask or alpha64");
    OCC_REQUIRE((image == nullptr) == (img64 == nullptr), "resize_frame: image and img64 come together (both or neither)");
    OCC_REQUIRE(image == nullptr || h_bgcolor, "resize_frame: null h_bgcolor with an image");
    OCC_REQUIRE(x_off_lanczos && x_w_lanczos && y_off_lanczos && y_w_lanczos && x_off_bilinear && x_w_bilinear &&
                    y_off_bilinear && y_w_bilinear,
                "resize_frame: null device table");
    OCC_REQUIRE(h_x_off_lanczos && h_y_off_lanczos && h_x_off_bilinear && h_y_off_bilinear,
                "resize_frame: null host copy of an offset table");
    OCC_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < (1ll << 28), "resize_frame: bad source size %d x %d", H, W);
    OCC_REQUIRE(h > 0 && w > 0 && (int64_t)h * w < (1ll << 28), "resize_frame: bad destination size %d x %d", h, w);
    int64_t bad;
    OCC_REQUIRE((bad = bad_offset(h_x_off_lanczos, (int64_t)w * kLanczos, W)) < 0,
                "resize_frame: x_off_lanczos[%lld] = %d reads outside the %d columns of the image", (long long)bad,
                h_x_off_lanczos[bad], W);
    OCC_REQUIRE((bad = bad_offset(h_x_off_bilinear, (int64_t)w * kLinear, W)) < 0,
                "resize_frame: x_off_bilinear[%lld] = %d reads outside the %d columns of the image", (long long)bad,
                h_x_off_bilinear[bad], W);
    OCC_REQUIRE((bad = bad_offset(h_y_off_lanczos, (int64_t)h * kLanczos, H)) < 0,
                "resize_frame: y_off_lanczos[%lld] = %d reads outside the %d rows of the image", (long long)bad,
                h_y_off_lanczos[bad], H);
    OCC_REQUIRE((bad = bad_offset(h_y_off_bilinear, (int64_t)h * kLinear, H)) < 0,
                "resize_frame: y_off_bilinear[%lld] = %d reads outside the %d rows of the image", (long long)bad,
                h_y_off_bilinear[bad], H);
    int tile_h = kTileH, span;                                    // the tallest tile whose source rows fit the LDS rows
    while ((span = tile_span(h_y_off_lanczos, h_y_off_bilinear, h, tile_h)) > kRows && tile_h > 1) tile_h--;
    OCC_REQUIRE(span <= kRows, "resize_frame: the y offsets of one output row span more than %d source rows or do not ascend",
                kRows);
    OCC_REQUIRE((h + tile_h - 1) / tile_h <= 65535, "resize_frame: %d output rows in tiles of %d rows are more than 65535 tiles",
                h, tile_h);
    const ResizeTables tb{x_off_lanczos, y_off_lanczos, x_off_bilinear, y_off_bilinear,
                          x_w_lanczos,   y_w_lanczos,   x_w_bilinear,   y_w_bilinear};
    const dim3 grid((w + kTileW - 1) / kTileW, (h + tile_h - 1) / tile_h);
    hipStream_t st = as_stream(stream);
    if (image)
        hipLaunchKernelGGL(resize_kernel<true>, grid, dim3(kBatchThreads), 0, st, image, mask, H, W, h, w, tile_h, tb,
                           (double)h_bgcolor[0], (double)h_bgcolor[1], (double)h_bgcolor[2], img64, alpha64);
    else
        hipLaunchKernelGGL(resize_kernel<false>, grid, dim3(kBatchThreads), 0, st, image, mask, H, W, h, w, tile_h, tb, 0.0,
                           0.0, 0.0, img64, alpha64);
    return check_launch("resize_frame");
}
