// What the three dataset-frame builders share (batch.hip: the training patch batch; frame.hip: the whole frame; view.hip: the
// rays of a camera without a photograph): the 256-thread workgroup's reductions and scans, the lane prefix of a wave64
// ballot, the store of one ray row, the reference's float64 blend and its 8-bit quantisation.  One definition of each, so
// the builders cannot drift apart.
#pragma once

#include "common.h"

namespace occ {

constexpr int kBatchThreads = 256;
constexpr int kBatchWaves = kBatchThreads / kWave;

__device__ __forceinline__ int lane_prefix(unsigned long long ballot) {      // set bits of the lanes below this one
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// Sum over the workgroup of a per-thread flag count; every thread gets the total.  `red` holds kBatchWaves ints.
__device__ __forceinline__ int block_sum(int v, int *red) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                   // red may still be read from the previous use
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < kBatchWaves; w++) s += red[w];
    return s;
}

// Exclusive prefix of `v` in thread order and the workgroup total.
__device__ __forceinline__ int block_excl_scan(int v, int *red, int &total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == kWave - 1) red[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kBatchWaves; w++) {
        if (w < wave) before += red[w];
        all += red[w];
    }
    total = all;
    return before + inc - v;
}

// Ordered compaction of one chunk of kBatchThreads flags: the number of set flags in the threads below this one, and the
// chunk's total.  Every thread of the workgroup calls it.
__device__ __forceinline__ int chunk_rank(bool hit, int *red, int &chunk) {
    const int t = threadIdx.x;
    const unsigned long long ballot = __ballot(hit);
    __syncthreads();                                   // red: the previous chunk's reads are done
    if ((t & (kWave - 1)) == 0) red[t / kWave] = __popcll(ballot);
    __syncthreads();
    int wave_off = 0;
    chunk = 0;
#pragma unroll
    for (int w = 0; w < kBatchWaves; w++) {
        if (w < t / kWave) wave_off += red[w];
        chunk += red[w];
    }
    return wave_off + lane_prefix(ballot);
}

// One ray row from the pixel's entry of rays8 (origin[3], direction[3], near, far): the origin to rays[0][row], the direction
// to rays[1][row] of rays[2][n_rows][3], near and far to their columns.
__device__ __forceinline__ void store_ray_row(const float *r8, int64_t row, int64_t n_rows, float *rays, float *near,
                                              float *far) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
        rays[row * 3 + c] = r8[c];
        rays[(n_rows + row) * 3 + c] = r8[3 + c];
    }
    near[row] = r8[6];
    far[row] = r8[7];
}

// train.py:296-297, :398 for one channel, in float64 with one rounding per operator (the tree is built with
// -ffp-contract=off): ((m / 255.) * image + (1.0 - m / 255.) * bgcolor) / 255. -> float32.
__device__ __forceinline__ float blend_target(uint8_t m, uint8_t image, double bg) {
    const double a = __ddiv_rn((double)m, 255.0);
    const double fg = __dmul_rn(a, (double)image);
    const double bk = __dmul_rn(__dsub_rn(1.0, a), bg);
    return (float)__ddiv_rn(__dadd_rn(fg, bk), 255.0);
}

// Where batch.hip and frame.hip read a frame's pixels from: the template parameter of their kernels.  p is the flat pixel
// index, c the channel.
//   subject(p)       the pixel belongs to the subject (train.py:470: alpha channel 0 > 0)
//   target(p, c, bg) the training target, float32 in 0..1 (:398)
//   alpha(p, c)      ray_alpha, float64
//   alpha0(p)        gt_alpha: float32 of the mask's channel 0
// PixelsU8: the resident uint8 photograph and mask, blended per pixel.
struct PixelsU8 {
    const uint8_t *__restrict__ image, *__restrict__ mask;
    __device__ __forceinline__ bool subject(size_t p) const { return mask[p * 3] > 0; }
    __device__ __forceinline__ float target(size_t p, int c, double bg) const {
        return blend_target(mask[p * 3 + c], image[p * 3 + c], bg);
    }
    __device__ __forceinline__ double alpha(size_t p, int c) const { return __ddiv_rn((double)mask[p * 3 + c], 255.0); }
    __device__ __forceinline__ float alpha0(size_t p) const { return (float)__ddiv_rn((double)mask[p * 3], 255.0); }
};

// PixelsF64: a frame occnerf_resize_frame has resized: img64 is the blend before its division by
// 255, already over the background, and alpha64 the resized mask / 255.
struct PixelsF64 {
    const double *__restrict__ img64, *__restrict__ alpha64;
    __device__ __forceinline__ bool subject(size_t p) const { return alpha64[p * 3] > 0.0; }
    __device__ __forceinline__ float target(size_t p, int c, double) const { return (float)__ddiv_rn(img64[p * 3 + c], 255.0); }
    __device__ __forceinline__ double alpha(size_t p, int c) const { return alpha64[p * 3 + c]; }
    __device__ __forceinline__ float alpha0(size_t p) const { return (float)alpha64[p * 3]; }
};

// image_util.py:19-20 to_8b_image: (255. * clip(x, 0, 1)).astype(uint8) in float32, truncation.
__device__ __forceinline__ uint8_t to_8b(float x) {
    x = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);          // np.clip (NaN propagates in numpy; not produced by the renderer)
    return (uint8_t)__fmul_rn(255.0f, x);
}

}  // namespace occ
