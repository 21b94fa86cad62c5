// What the two v_mfma_f32_16x16x4_f32 kernels (mlp16.hip at width 256, nonrigid16.hip at width 128) share: the layer's
// epilogue on a tile's registers.  A tile is 16 samples; lane (g = l >> 4, s = l & 15) holds in register r of output block
// ob the feature 16 ob + 4 g + r of sample s (mlp16.hip: layout), so a width-W layer is OB = W / 16 registers of f32x4.
#pragma once

#include "common.h"

namespace occ {

constexpr int groups_of(int ks) { return (ks + 3) / 4; }      // chunk groups of 4 k-steps

// acc = the layer's bias (torch order, in LDS)
template <int OB>
__device__ __forceinline__ void lds_bias(f32x4 (&acc)[OB], const float *aux, int g) {
    const f32x4 *B4 = reinterpret_cast<const f32x4 *>(aux);
#pragma unroll
    for (int ob = 0; ob < OB; ob++) acc[ob] = B4[ob * 4 + g];
}

template <int OB>
__device__ __forceinline__ void relu_into(f32x4 (&act)[OB], const f32x4 (&acc)[OB]) {
#pragma unroll
    for (int ob = 0; ob < OB; ob++) {
#pragma unroll
        for (int r = 0; r < 4; r++) act[ob][r] = relu_arith(acc[ob][r]);
    }
}

// dot product of a torch-layout weight row (in LDS) with the lane's 4 OB activations (features 16*ob+4*g+r), an fma chain
// in that order from 0; the other three quarters live in the lanes s+16, s+32, s+48
template <int OB>
__device__ __forceinline__ float dot_row(const f32x4 (&act)[OB], const float *Wrow, int g) {
    const f32x4 *W4 = reinterpret_cast<const f32x4 *>(Wrow);
    float s = 0.0f;
#pragma unroll
    for (int ob = 0; ob < OB; ob++) {
        const f32x4 w = W4[ob * 4 + g];
#pragma unroll
        for (int r = 0; r < 4; r++) s = __fmaf_rn(w[r], act[ob][r], s);
    }
    s += __shfl_xor(s, 16);
    return s + __shfl_xor(s, 32);
}

}  // namespace occ
