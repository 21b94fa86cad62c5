// Per-frame image metrics of the reference's eval.py:100-218 -- SSIM (skimage.metrics.structural_similarity with
// multichannel=True on float64 images), PSNR over three pixel selections and the silhouette IoU -- on the 8-bit images
// that unpack_to_image builds.
//
// The inputs are 8-bit, so the 7x7 box sums of x, y, x^2, y^2 and xy are exact integers (the largest, 49 * 255^2 =
// 3 186 225, fits int32), and so are the centred numerators c_xy = 49 S_xy - S_x S_y (|c| <= 49^2 * 255^2 / 4 < 2^31).
// skimage's float64 S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), with ux = S_x / (49 * 255) and
// v = 49/48 * c / (49 * 255)^2, is then (every factor multiplied by (49 * 255)^2, which cancels)
//     S = (2 S_x S_y + c1)(49/48 * 2 c_xy + c2) / ((S_x^2 + S_y^2 + c1)(49/48 (c_xx + c_yy) + c2)),
//     c1 = C1 (49 * 255)^2,  c2 = C2 (49 * 255)^2,
// evaluated in fp64 from exact integers: no cancellation anywhere, and identical images give S == 1.0 exactly (numerator
// and denominator are the same operations on the same integers).
//
// Kernel 1: one workgroup per 64 x 16 output tile of one frame.  The (64 + 6) x (16 + 6) halo of both images is staged
// in LDS, planar per channel, with scipy.ndimage's 'reflect' indexing at the border (half-sample symmetric; skimage
// requires H, W >= 7, so one reflection always suffices).  Per channel: a horizontal 7-tap pass of the five integer moments
// into LDS, then a vertical one per output pixel, S in fp64, and every per-frame sum of eval.py accumulated on the spot:
// the cropped S sum (mssim), the S sums over the body and vis masks, the integer squared-error sums over full / body / vis,
// the pixel counts and the IoU intersection and union.  Each workgroup writes one MetricsPartial.
// Kernel 2: one workgroup per frame sums its tiles' partials in a fixed order and writes the frame's fp64 record.  There
// are no atomics, so the results are bitwise deterministic and independent of the batch size.
#include "common.h"

namespace occ {

constexpr int kMetTW = 64, kMetTH = 16;                  // output tile
constexpr int kMetHW = kMetTW + 6, kMetHH = kMetTH + 6;  // halo tile
constexpr int kMetThreads = 256;                         // 64 columns x 4 groups of 4 rows
constexpr int kMetRows = kMetTH / (kMetThreads / kMetTW);
constexpr int kMetRecord = OCCNERF_FRAME_METRICS_RECORD;

struct MetricsPartial {
    double s_crop, s_body, s_vis;                       // S summed over channels and the pixels of each selection
    long long sse_full, sse_body, sse_vis;              // sum of (x - y)^2 in 8-bit units, over channels
    long long n_body, n_vis, inter, uni;                // pixel counts
};

__device__ __forceinline__ int met_reflect(int i, int n) {
    if (i < 0) i = -i - 1;                              // scipy 'reflect': d c b a | a b c d | d c b a
    if (i >= n) i = 2 * n - 1 - i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);            // clamp: halo positions that feed no output pixel
}

template <typename T>
__device__ __forceinline__ T met_wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__global__ __launch_bounds__(kMetThreads) void frame_metrics_tile_kernel(
    const uint8_t *__restrict__ pred, const uint8_t *__restrict__ truth, const float *__restrict__ alpha,
    const uint8_t *__restrict__ body, const float *__restrict__ gt_vis, const float *__restrict__ gt_alpha, int H, int W,
    int tiles_x, double c1, double c2, double *__restrict__ smap, MetricsPartial *__restrict__ part) {
    __shared__ uint8_t lx[3][kMetHH][kMetHW], ly[3][kMetHH][kMetHW];
    __shared__ int m_x[kMetHH][kMetTW], m_y[kMetHH][kMetTW], m_xx[kMetHH][kMetTW], m_yy[kMetHH][kMetTW],
        m_xy[kMetHH][kMetTW];
    __shared__ double red_d[kMetThreads / 64][3];
    __shared__ long long red_i[kMetThreads / 64][7];

    const int tid = threadIdx.x, n = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int r0 = ty * kMetTH, c0 = tx * kMetTW;
    const int64_t npx = (int64_t)H * W;
    const uint8_t *P = pred + n * npx * 3, *T = truth + n * npx * 3;

    for (int i = tid; i < kMetHH * kMetHW * 3; i += kMetThreads) {    // consecutive lanes: consecutive bytes of a row
        const int pix = i / 3, c = i - pix * 3;
        const int hr = pix / kMetHW, hc = pix - hr * kMetHW;
        const int64_t off = ((int64_t)met_reflect(r0 - 3 + hr, H) * W + met_reflect(c0 - 3 + hc, W)) * 3 + c;
        lx[c][hr][hc] = P[off];
        ly[c][hr][hc] = T[off];
    }

    // this thread's pixels: one column, kMetRows rows; the masks are per pixel (all three channels share them)
    const int col = tid % kMetTW, row0 = (tid / kMetTW) * kMetRows, cc = c0 + col;
    bool valid[kMetRows], in_crop[kMetRows], in_body[kMetRows], in_vis[kMetRows];
    long long n_body = 0, n_vis = 0, inter = 0, uni = 0;
#pragma unroll
    for (int j = 0; j < kMetRows; j++) {
        const int r = r0 + row0 + j;
        valid[j] = r < H && cc < W;
        in_crop[j] = valid[j] && r >= 3 && r < H - 3 && cc >= 3 && cc < W - 3;
        in_body[j] = in_vis[j] = false;
        if (!valid[j]) continue;
        const int64_t p = n * npx + (int64_t)r * W + cc;
        const float a = alpha ? alpha[p] : 0.0f;
        in_body[j] = body && body[p] != 0;
        in_vis[j] = gt_vis ? gt_vis[p] > 0.5f : a > 0.001f;    // float32 comparisons, as numpy makes them
        n_body += in_body[j];
        n_vis += in_vis[j];
        if (gt_alpha) {
            const bool pm = a > 0.1f, gm = gt_alpha[p] > 0.5f;
            inter += pm && gm;
            uni += pm || gm;
        }
    }

    double s_crop = 0.0, s_body = 0.0, s_vis = 0.0;
    long long sse_full = 0, sse_body = 0, sse_vis = 0;
    for (int c = 0; c < 3; c++) {
        __syncthreads();                                // halo staged / previous channel's moments consumed
        for (int i = tid; i < kMetHH * kMetTW; i += kMetThreads) {
            const int hr = i / kMetTW, hc = i - hr * kMetTW;
            int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
            for (int k = 0; k < 7; k++) {
                const int a = lx[c][hr][hc + k], b = ly[c][hr][hc + k];
                sx += a;
                sy += b;
                sxx += a * a;
                syy += b * b;
                sxy += a * b;
            }
            m_x[hr][hc] = sx;
            m_y[hr][hc] = sy;
            m_xx[hr][hc] = sxx;
            m_yy[hr][hc] = syy;
            m_xy[hr][hc] = sxy;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kMetRows; j++) {
            if (!valid[j]) continue;
            const int row = row0 + j;
            int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
            for (int k = 0; k < 7; k++) {
                sx += m_x[row + k][col];
                sy += m_y[row + k][col];
                sxx += m_xx[row + k][col];
                syy += m_yy[row + k][col];
                sxy += m_xy[row + k][col];
            }
            const long long pxy = (long long)sx * sy;
            const long long cxy2 = 2 * (49LL * sxy - pxy);
            const long long cvv = (49LL * sxx - (long long)sx * sx) + (49LL * syy - (long long)sy * sy);
            const double a1 = (double)(2 * pxy) + c1;
            const double b1 = (double)((long long)sx * sx + (long long)sy * sy) + c1;
            const double a2 = 49.0 * (double)cxy2 / 48.0 + c2;
            const double b2 = 49.0 * (double)cvv / 48.0 + c2;
            const double S = (a1 * a2) / (b1 * b2);
            const int64_t p = n * npx + (int64_t)(r0 + row) * W + cc;
            if (smap) smap[p * 3 + c] = S;
            const int d = (int)lx[c][row + 3][col + 3] - (int)ly[c][row + 3][col + 3];
            sse_full += d * d;
            if (in_crop[j]) s_crop += S;
            if (in_body[j]) {
                s_body += S;
                sse_body += d * d;
            }
            if (in_vis[j]) {
                s_vis += S;
                sse_vis += d * d;
            }
        }
    }

    // workgroup sums in a fixed order: a shuffle tree per wave, then the waves in index order
    s_crop = met_wave_sum(s_crop);
    s_body = met_wave_sum(s_body);
    s_vis = met_wave_sum(s_vis);
    sse_full = met_wave_sum(sse_full);
    sse_body = met_wave_sum(sse_body);
    sse_vis = met_wave_sum(sse_vis);
    n_body = met_wave_sum(n_body);
    n_vis = met_wave_sum(n_vis);
    inter = met_wave_sum(inter);
    uni = met_wave_sum(uni);
    const int wave = tid / 64;
    if ((tid & 63) == 0) {
        red_d[wave][0] = s_crop;
        red_d[wave][1] = s_body;
        red_d[wave][2] = s_vis;
        red_i[wave][0] = sse_full;
        red_i[wave][1] = sse_body;
        red_i[wave][2] = sse_vis;
        red_i[wave][3] = n_body;
        red_i[wave][4] = n_vis;
        red_i[wave][5] = inter;
        red_i[wave][6] = uni;
    }
    __syncthreads();
    if (tid == 0) {
        MetricsPartial q = {};
        for (int w = 0; w < kMetThreads / 64; w++) {
            q.s_crop += red_d[w][0];
            q.s_body += red_d[w][1];
            q.s_vis += red_d[w][2];
            q.sse_full += red_i[w][0];
            q.sse_body += red_i[w][1];
            q.sse_vis += red_i[w][2];
            q.n_body += red_i[w][3];
            q.n_vis += red_i[w][4];
            q.inter += red_i[w][5];
            q.uni += red_i[w][6];
        }
        part[(int64_t)n * gridDim.x + blockIdx.x] = q;
    }
}

// eval.py:87-91 psnr_metric: mse = mean((a/255 - b/255)^2) over the selected elements, psnr = -10 * log(mse) / log(10);
// numpy's float64 semantics: 0 / 0 = nan for an empty selection, log(0) = -inf -> inf for mse = 0
__device__ __forceinline__ double met_psnr(long long sse, long long n_px) {
    const double mse = ((double)sse / 65025.0) / (3.0 * (double)n_px);
    return -10.0 * log(mse) / log(10.0);
}

__global__ __launch_bounds__(kMetThreads) void frame_metrics_finish_kernel(const MetricsPartial *__restrict__ part,
                                                                           int tiles, int H, int W,
                                                                           double *__restrict__ record) {
    __shared__ MetricsPartial red[kMetThreads];
    const int tid = threadIdx.x, n = blockIdx.x;
    MetricsPartial q = {};
    for (int t = tid; t < tiles; t += kMetThreads) {   // fixed order per thread
        const MetricsPartial &s = part[(int64_t)n * tiles + t];
        q.s_crop += s.s_crop;
        q.s_body += s.s_body;
        q.s_vis += s.s_vis;
        q.sse_full += s.sse_full;
        q.sse_body += s.sse_body;
        q.sse_vis += s.sse_vis;
        q.n_body += s.n_body;
        q.n_vis += s.n_vis;
        q.inter += s.inter;
        q.uni += s.uni;
    }
    red[tid] = q;
    for (int h = kMetThreads / 2; h > 0; h >>= 1) {   // fixed tree
        __syncthreads();
        if (tid < h) {
            MetricsPartial &a = red[tid];
            const MetricsPartial &b = red[tid + h];
            a.s_crop += b.s_crop;
            a.s_body += b.s_body;
            a.s_vis += b.s_vis;
            a.sse_full += b.sse_full;
            a.sse_body += b.sse_body;
            a.sse_vis += b.sse_vis;
            a.n_body += b.n_body;
            a.n_vis += b.n_vis;
            a.inter += b.inter;
            a.uni += b.uni;
        }
    }
    if (tid != 0) return;
    const MetricsPartial &t = red[0];
    double *rec = record + (int64_t)n * kMetRecord;
    rec[0] = met_psnr(t.sse_vis, t.n_vis);
    rec[1] = t.s_vis / (3.0 * (double)t.n_vis);
    rec[2] = met_psnr(t.sse_body, t.n_body);
    rec[3] = t.s_body / (3.0 * (double)t.n_body);
    rec[4] = met_psnr(t.sse_full, (long long)H * W);
    rec[5] = t.s_crop / (3.0 * (double)(H - 6) * (double)(W - 6));
    rec[6] = (double)t.inter / (double)t.uni;
    rec[7] = (double)t.n_vis;
    rec[8] = (double)t.n_body;
    rec[9] = (double)t.inter;
    rec[10] = (double)t.uni;
    rec[11] = (double)t.sse_vis;
    rec[12] = (double)t.sse_body;
    rec[13] = (double)t.sse_full;
}

static int met_tiles(int32_t H, int32_t W, int *tiles_x) {
    *tiles_x = (W + kMetTW - 1) / kMetTW;
    return *tiles_x * ((H + kMetTH - 1) / kMetTH);
}

static bool met_sizes_ok(int32_t N, int32_t H, int32_t W) {
    return N >= 1 && N <= 65535 && H >= 7 && W >= 7 && H <= (1 << 15) && W <= (1 << 15);
}

}  // namespace occ

OCC_API int64_t occnerf_frame_metrics_workspace_bytes(int32_t N, int32_t H, int32_t W) {
    using namespace occ;
    if (!met_sizes_ok(N, H, W)) return -1;
    int tx;
    return (int64_t)N * met_tiles(H, W, &tx) * (int64_t)sizeof(MetricsPartial);
}

OCC_API int occnerf_frame_metrics(const uint8_t *pred, const uint8_t *truth, const float *alpha, const uint8_t *body,
                                  const float *gt_vis_alpha, const float *gt_alpha, int32_t N, int32_t H, int32_t W,
                                  double data_range, double *record, double *ssim_map, void *workspace, void *stream) {
    using namespace occ;
    OCC_REQUIRE(pred && truth && record && workspace, "frame_metrics: null argument (pred, truth, record and workspace are required)");
    OCC_REQUIRE(met_sizes_ok(N, H, W), "frame_metrics: bad sizes N=%d H=%d W=%d (1 <= N <= 65535, 7 <= H, W <= 32768)", N, H,
                W);
    OCC_REQUIRE(data_range > 0.0 && data_range < 1e300, "frame_metrics: data_range must be positive and finite");
    int tiles_x;
    const int tiles = met_tiles(H, W, &tiles_x);
    const double d0 = 49.0 * 255.0;                     // the integer moments are (49 * 255) x the float64 means
    const double c1 = (0.01 * data_range) * (0.01 * data_range) * d0 * d0;
    const double c2 = (0.03 * data_range) * (0.03 * data_range) * d0 * d0;
    MetricsPartial *part = static_cast<MetricsPartial *>(workspace);
    hipLaunchKernelGGL(frame_metrics_tile_kernel, dim3((unsigned)tiles, (unsigned)N), dim3(kMetThreads), 0, as_stream(stream),
                       pred, truth, alpha, body, gt_vis_alpha, gt_alpha, (int)H, (int)W, tiles_x, c1, c2, ssim_map, part);
    int rc = check_launch("frame_metrics tiles");
    if (rc) return rc;
    hipLaunchKernelGGL(frame_metrics_finish_kernel, dim3((unsigned)N), dim3(kMetThreads), 0, as_stream(stream), part, tiles,
                       (int)H, (int)W, record);
    return check_launch("frame_metrics finish");
}
