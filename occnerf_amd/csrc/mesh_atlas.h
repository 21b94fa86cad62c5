// The per-triangle atlas of the exported mesh, as the kernels that write or read it share it
// (mesh_texture.hip, mesh_normal.hip): the limits, texel k of a triangle in its own frame, a texel's place in the atlas, the walk
// of the kernels that run one thread per owned texel, the bilinear sampler of the resolves, and the refusals every entry on the
// atlas makes before it launches.  Triangles 2c and 2c + 1 share the n x n cell c; the even one owns the texels i + j <= n - 2
// of the cell, the odd one those of the mirrored frame i' = n - 1 - i, j' = n - 1 - j; every triangle owns P = n (n - 1) / 2
// texels, numbered by ascending j', then ascending i'.  The sampler is fp64 with + - * floor and comparisons only, one rounding
// per operator in the order of tests/mesh_texture_restatement.py.
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

// Owned texel g of T P -> its triangle t; (i', j') in the triangle's frame and (x, y) in the atlas.
__device__ __forceinline__ int64_t texel_walk(int64_t g, int n, int P, int C, int &i, int &j, int &x, int &y) {
    const int64_t t = g / P;
    texel_of((int)(g - t * P), n, i, j);
    atlas_of(t, i, j, n, C, x, y);
    return t;
}

// Section 7o's sampler: the four texels of triangle t around the weights (w1, w2) of its vertices 1 and 2, all of them t's own.
struct AtlasTaps {
    const uint8_t *c00, *c10, *c01, *c11;
    double w00, w10, w01, w11;
    // The unrounded blend of channel c.
    __device__ __forceinline__ double blend(int c) const {
        return ((w00 * (double)c00[c] + w10 * (double)c10[c]) + w01 * (double)c01[c]) + w11 * (double)c11[c];
    }
};

__device__ __forceinline__ AtlasTaps atlas_taps(const uint8_t *__restrict__ atlas, int aW, int64_t t, double w1, double w2, int n,
                                                int C) {
    const double dm = (double)(n - 3);
    const double xr = w1 * dm, yr = w2 * dm;
    const double x = xr > 0.0 ? (xr < dm ? xr : dm) : 0.0;
    const double ym = dm - x;
    const double y = yr > 0.0 ? (yr < ym ? yr : ym) : 0.0;
    const double fx = floor(x), fy = floor(y);
    const double ax = x - fx, ay = y - fy;
    const int i0 = (int)fx, j0 = (int)fy;
    const int i1 = i0 + 1 < n ? i0 + 1 : n - 1, j1 = j0 + 1 < n ? j0 + 1 : n - 1;      // (0 <= i0, j0 <= n - 3)
    int x00, y00, x10, y10, x01, y01, x11, y11;
    atlas_of(t, i0, j0, n, C, x00, y00);
    atlas_of(t, i1, j0, n, C, x10, y10);
    atlas_of(t, i0, j1, n, C, x01, y01);
    atlas_of(t, i1, j1, n, C, x11, y11);
    AtlasTaps s;
    s.c00 = atlas + ((int64_t)y00 * aW + x00) * 3, s.c10 = atlas + ((int64_t)y10 * aW + x10) * 3;
    s.c01 = atlas + ((int64_t)y01 * aW + x01) * 3, s.c11 = atlas + ((int64_t)y11 * aW + x11) * 3;
    s.w00 = (1.0 - ax) * (1.0 - ay), s.w10 = ax * (1.0 - ay), s.w01 = (1.0 - ax) * ay, s.w11 = ax * ay;
    return s;
}

// The refusals of the entries on the atlas, `who` the entry's name: false with the error text set.
inline bool tex_cell_ok(const char *who, int32_t n) {
    if (n >= kTexMinCell && n <= kTexMaxCell) return true;
    set_error("%s: n=%d outside %d..%d", who, n, kTexMinCell, kTexMaxCell);
    return false;
}

// P = n (n - 1) / 2 of a checked n comes back; T >= 0 and T P < 2^31.
inline bool tex_count_ok(const char *who, int64_t T, int32_t n, int64_t &P) {
    P = (int64_t)n * (n - 1) / 2;
    if (T >= 0 && T < (1ll << 31) && T * P < (1ll << 31)) return true;
    set_error("%s: T=%lld with %lld texels each reaches 2^31", who, (long long)T, (long long)P);
    return false;
}

// The cells of T triangles fit an atlas of C cells per row and H rows of texels.
inline bool tex_atlas_ok(const char *who, int64_t T, int32_t n, int32_t C, int32_t H, int32_t W) {
    const int64_t cells = (T + 1) / 2, rows = C < 1 ? 0 : (cells + C - 1) / C;
    if (C >= 1 && W == (int64_t)C * n && H >= 1 && H <= kTexMaxSide && W <= kTexMaxSide && rows * n <= H) return true;
    set_error("%s: an atlas of H=%d W=%d with C=%d cells of %d per row does not hold T=%lld triangles (W = C n, rows of cells * n "
              "<= H <= %d)", who, H, W, C, n, (long long)T, kTexMaxSide);
    return false;
}

}  // namespace occ
