// The per-triangle atlas of the exported mesh, as the kernels that write or read it share it
// (mesh_texture.hip, mesh_normal.hip): the limits, texel k of a triangle in its own frame, a texel's place in the atlas and the
// test that an atlas holds T triangles.  Triangles 2c and 2c + 1 share the n x n cell c; the even one owns the texels
// i + j <= n - 2 of the cell, the odd one those of the mirrored frame i' = n - 1 - i, j' = n - 1 - j; every triangle owns
// P = n (n - 1) / 2 texels, numbered by ascending j', then ascending i'.
#pragma once

#include "common.h"

namespace occ {

constexpr int kTexThreads = 256;
constexpr int kTexMinCell = 4;
constexpr int kTexMaxCell = 64;
constexpr int kTexMaxSide = 16384;

// Texel k of a triangle -> (i', j') in its own frame: row j' holds the n - 1 - j' texels i' = 0 .. n - 2 - j'.
__device__ __forceinline__ void texel_of(int k, int n, int &i, int &j) {
    int row = n - 1;
    j = 0;
    while (k >= row) {              // at most n - 2 <= 62 steps
        k -= row;
        row--;
        j++;
    }
    i = k;
}

// (column, row) in the atlas of texel (i', j') of triangle t.
__device__ __forceinline__ void atlas_of(int64_t t, int i, int j, int n, int C, int &x, int &y) {
    const int64_t c = t >> 1;
    const bool odd = (t & 1) != 0;
    x = (int)(c % C) * n + (odd ? n - 1 - i : i);
    y = (int)(c / C) * n + (odd ? n - 1 - j : j);
}

// The cells of T triangles fit an atlas of C cells per row and H rows of texels.
inline bool tex_layout_ok(int64_t T, int32_t n, int32_t C, int32_t H, int32_t W) {
    if (C < 1 || W != (int64_t)C * n || H < 1 || H > kTexMaxSide || W > kTexMaxSide) return false;
    const int64_t cells = (T + 1) / 2, rows = (cells + C - 1) / C;
    return rows * n <= H;
}

}  // namespace occ
