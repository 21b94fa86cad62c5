// Undistorting a frame of a prepared dataset when it is opened (the reference's cv2.undistort lines, core/data/occnerf/
// train.py:290-294 and allview.py:166-170): occnerf_amd/undistort.py's undistort_u8 on the device, bit for bit.  That is
// OpenCV's undistort -> initUndistortRectifyMap (CV_16SC2, 1/32-pixel fractions) -> remap (INTER_LINEAR, BORDER_CONSTANT 0)
// with the camera matrix kept, restated as a pure function of its inputs.
//
// One thread per pixel of the output window: the map of the pixel once, in float64 with one rounding per operator (the tree
// is built with -ffp-contract=off; the operators are spelt __d*_rn as batch_common.h's blend is), then four taps of three
// channels from the photograph and, when there is one, from the mask -- six channels from one map.  The weights are
// integers that sum to 1024, so a channel is (acc + 512) >> 10 in int32.  A tap outside the image reads 0, tested per tap;
// only the window is written, with plain byte stores; no atomics, no LDS.
#include "batch_common.h"

namespace occ {

struct UndistortCamera {
    double fx, fy, cx, cy;
    double k1, k2, p1, p2, k3, k4, k5, k6;
};

// rint(32 * c): ties to even, saturated to int32.  `c` is finite.
__device__ __forceinline__ int fixed5(double c) {
    double s = rint(__dmul_rn(c, 32.0));
    s = s < -2147483648.0 ? -2147483648.0 : (s > 2147483647.0 ? 2147483647.0 : s);
    return (int)s;
}

__global__ __launch_bounds__(kBatchThreads) void undistort_kernel(const uint8_t *__restrict__ image,
                                                                 const uint8_t *__restrict__ mask, int H, int W,
                                                                 UndistortCamera cam, int win_y, int win_x, int win_h,
                                                                 int win_w, uint8_t *__restrict__ out_image,
                                                                 uint8_t *__restrict__ out_mask) {
    const int q = blockIdx.x * kBatchThreads + threadIdx.x;          // win_h * win_w <= H * W < 2^28
    if (q >= win_h * win_w) return;
    const int i = win_y + q / win_w, j = win_x + q % win_w;
    const double x = __ddiv_rn(__dsub_rn((double)j, cam.cx), cam.fx);
    const double y = __ddiv_rn(__dsub_rn((double)i, cam.cy), cam.fy);
    const double x2 = __dmul_rn(x, x), y2 = __dmul_rn(y, y);
    const double r2 = __dadd_rn(x2, y2);
    const double _2xy = __dmul_rn(__dmul_rn(2.0, x), y);
    const double num = __dadd_rn(1.0, __dmul_rn(__dadd_rn(__dmul_rn(__dadd_rn(__dmul_rn(cam.k3, r2), cam.k2), r2), cam.k1), r2));
    const double den = __dadd_rn(1.0, __dmul_rn(__dadd_rn(__dmul_rn(__dadd_rn(__dmul_rn(cam.k6, r2), cam.k5), r2), cam.k4), r2));
    const double kr = __ddiv_rn(num, den);
    const double xd = __dadd_rn(__dadd_rn(__dmul_rn(x, kr), __dmul_rn(cam.p1, _2xy)),
                                __dmul_rn(cam.p2, __dadd_rn(r2, __dmul_rn(2.0, x2))));
    const double yd = __dadd_rn(__dadd_rn(__dmul_rn(y, kr), __dmul_rn(cam.p1, __dadd_rn(r2, __dmul_rn(2.0, y2)))),
                                __dmul_rn(cam.p2, _2xy));
    const double u = __dadd_rn(__dmul_rn(cam.fx, xd), cam.cx);
    const double v = __dadd_rn(__dmul_rn(cam.fy, yd), cam.cy);
    const bool finite = isfinite(u) && isfinite(v);
    const int iu = finite ? fixed5(u) : 0, iv = finite ? fixed5(v) : 0;
    const int x0 = iu >> 5, a = iu & 31, y0 = iv >> 5, b = iv & 31;      // arithmetic shifts; |x0| < 2^26, so x0 + 1 is safe
    const bool in_x[2] = {x0 >= 0 && x0 < W, x0 + 1 >= 0 && x0 + 1 < W};
    const bool in_y[2] = {y0 >= 0 && y0 < H, y0 + 1 >= 0 && y0 + 1 < H};
    const int wgt[4] = {(32 - b) * (32 - a), (32 - b) * a, b * (32 - a), b * a};
    size_t tap[4];
    bool in[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        in[t] = finite && in_y[t >> 1] && in_x[t & 1];
        tap[t] = in[t] ? ((size_t)(y0 + (t >> 1)) * W + (x0 + (t & 1))) * 3 : 0;      // never formed from an outside tap
    }
    const size_t o = (size_t)q * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        int acc = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) acc += in[t] ? wgt[t] * (int)image[tap[t] + c] : 0;
        out_image[o + c] = (uint8_t)((acc + 512) >> 10);
    }
    if (mask == nullptr) return;                       // wave-uniform
#pragma unroll
    for (int c = 0; c < 3; c++) {
        int acc = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) acc += in[t] ? wgt[t] * (int)mask[tap[t] + c] : 0;
        out_mask[o + c] = (uint8_t)((acc + 512) >> 10);
    }
}

}  // namespace occ

OCC_API int occnerf_undistort_u8(const uint8_t *image, const uint8_t *mask, int32_t H, int32_t W, const double *h_K,
                                 const double *h_dist, int32_t win_y, int32_t win_x, int32_t win_h, int32_t win_w,
                                 uint8_t *out_image, uint8_t *out_mask, void *stream) {
    using namespace occ;
    OCC_REQUIRE(image && h_K && h_dist && out_image, "undistort_u8: null argument");
    OCC_REQUIRE((mask == nullptr) == (out_mask == nullptr), "undistort_u8: mask and out_mask come together (both or neither)");
    OCC_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < (1ll << 28), "undistort_u8: bad image size %d x %d", H, W);
    OCC_REQUIRE(win_h > 0 && win_w > 0 && win_y >= 0 && win_x >= 0 && (int64_t)win_y + win_h <= H &&
                    (int64_t)win_x + win_w <= W,
                "undistort_u8: window (y %d, x %d, %d x %d) is not inside the %d x %d image", win_y, win_x, win_w, win_h, W, H);
    OCC_REQUIRE(h_K[1] == 0.0, "undistort_u8: skew K[0,1] = %g is not built", h_K[1]);
    const UndistortCamera cam{h_K[0], h_K[4], h_K[2], h_K[5], h_dist[0], h_dist[1], h_dist[2], h_dist[3],
                              h_dist[4], h_dist[5], h_dist[6], h_dist[7]};
    const int blocks = (win_h * win_w + kBatchThreads - 1) / kBatchThreads;
    hipLaunchKernelGGL(undistort_kernel, dim3(blocks), dim3(kBatchThreads), 0, as_stream(stream), image, mask, H, W, cam,
                       win_y, win_x, win_h, win_w, out_image, out_mask);
    return check_launch("undistort_u8");
}
