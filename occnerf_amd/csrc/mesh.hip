// The body as a triangle mesh (occnerf_amd/mesh.py): marching tetrahedra on the Kuhn split of every cube
// of a float32 field[nz][ny][nx].  Each cube is cut into the six tetrahedra that share its body diagonal, one per permutation
// of the axes (x, y, z) in lexicographic order: tetrahedron t has the cube corners 0, e_p0, e_p0 + e_p1, 7 (corner c = dx +
// 2 dy + 4 dz).  A corner is inside iff f > level (strict, float32: NaN is outside).  A surface vertex lies on an edge that
// leaves a grid point in a non-negative direction d != 0 and is named by the key lo_linear * 7 + (dx + 2 dy + 4 dz - 1).
//   occnerf_mesh_count     one workgroup per row of cubes (z, y) walks x in chunks of 256 threads and writes the row's
//                          triangle count (0, 1 or 2 per tetrahedron);
//   occnerf_mesh_emit      the same walk; an LDS prefix sum of the per-thread counts across the four waves places every
//                          cube's triangles behind row_start[row], so they come out in the order (z, y, x, tetrahedron,
//                          triangle within the case), wound by kCaseTable: (b - a) x (c - a) points from inside to outside;
//   occnerf_mesh_vertices  one thread per welded key: the crossing of the level on the key's edge in fp64, one rounding per
//                          operator (the tree is built with -ffp-contract=off), rounded once to float32.
// The field is left to the caches: the eight corner loads of a wave are four runs of 65 consecutive floats, the x + 1 load
// hits the line the x load brought in, and the two point rows x two slabs of a cube row are the neighbouring workgroups' too
// (L2; a 257^3 field is 68 MB, inside the 256 MiB last-level cache).  Staging them in LDS would save one of two L1 hits per
// row and add a barrier per chunk.  No atomics, no host wait; every output is a pure function of the inputs.
#include "batch_common.h"

namespace occ {

constexpr int kMeshTets = 6;
constexpr int kMeshTableBytes = kMeshTets * 16 * 6;
constexpr uint8_t kMeshEmpty = 0xFF;

// The middle two corners of each tetrahedron's path 0 -> e_p0 -> e_p0 + e_p1 -> 7.
__device__ constexpr uint8_t kTetMid[kMeshTets][2] = {{1, 3}, {1, 5}, {2, 3}, {2, 6}, {4, 5}, {4, 6}};

// [tetrahedron][inside mask, bit i = corner i of the path][two triangles x three vertices]: corner * 8 + kind of the edge
// the vertex lies on (the cube corner at its lo end, its direction), kMeshEmpty where the case has no such triangle.  Built
// from the geometry of the unit cube by tests/mesh_restatement.py's case_table(), which the tests compare with these bytes.
__device__ const uint8_t kCaseTable[kMeshTableBytes] = {
    0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,      // tetrahedron 0, inside mask 0000
    0x00, 0x02, 0x06, 0xFF, 0xFF, 0xFF,      // tetrahedron 0, inside mask 0001
    0x00, 0x0D, 0x09, 0xFF, 0xFF, 0xFF,      // tetrahedron 0, inside mask 0010
    0x02, 0x06, 0x0D, 0x02, 0x0D, 0x09,      // tetrahedron 0, inside mask 0011
    0x02, 0x09, 0x1B, 0xFF, 0xFF, 0xFF,      // tetrahedron 0, inside mask 0100
    0x00, 0x1B, 0x06, 0x00, 0x09, 0x1B,      // tetrahedron 0, inside mask 0101
    0x00, 0x0D, 0x1B, 0x00, 0x1B, 0x02,      // tetrahedron 0, inside mask 0110
    0x06, 0x0D, 0x1B, 0xFF, 0xFF, 0xFF,      // tetrahedron 0, inside mask 0111
    0x06, 0x1B, 0x0D, 0xFF, 0xFF, 0xFF,      // tetrahedron 0, inside mask 1000
    0x00, 0x02, 0x1B, 0x00, 0x1B, 0x0D,      // tetrahedron 0, inside mask 1001
    0x00, 0x1B, 0x09, 0x00, 0x06, 0x1B,      // tetrahedron 0, inside mask 1010
    0x02, 0x1B, 0x09, 0xFF, 0xFF, 0xFF,      // tetrahedron 0, inside mask 1011
    0x02, 0x09, 0x0D, 0x02, 0x0D, 0x06,      // tetrahedron 0, inside mask 1100
    0x00, 0x09, 0x0D, 0xFF, 0xFF, 0xFF,      // tetrahedron 0, inside mask 1101
    0x00, 0x06, 0x02, 0xFF, 0xFF, 0xFF,      // tetrahedron 0, inside mask 1110
    0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,      // tetrahedron 0, inside mask 1111
    0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,      // tetrahedron 1, inside mask 0000
    0x00, 0x06, 0x04, 0xFF, 0xFF, 0xFF,      // tetrahedron 1, inside mask 0001
    0x00, 0x0B, 0x0D, 0xFF, 0xFF, 0xFF,      // tetrahedron 1, inside mask 0010
    0x04, 0x0D, 0x06, 0x04, 0x0B, 0x0D,      // tetrahedron 1, inside mask 0011
    0x04, 0x29, 0x0B, 0xFF, 0xFF, 0xFF,      // tetrahedron 1, inside mask 0100
    0x00, 0x06, 0x29, 0x00, 0x29, 0x0B,      // tetrahedron 1, inside mask 0101
    0x00, 0x29, 0x0D, 0x00, 0x04, 0x29,      // tetrahedron 1, inside mask 0110
    0x06, 0x29, 0x0D, 0xFF, 0xFF, 0xFF,      // tetrahedron 1, inside mask 0111
    0x06, 0x0D, 0x29, 0xFF, 0xFF, 0xFF,      // tetrahedron 1, inside mask 1000
    0x00, 0x29, 0x04, 0x00, 0x0D, 0x29,      // tetrahedron 1, inside mask 1001
    0x00, 0x0B, 0x29, 0x00, 0x29, 0x06,      // tetrahedron 1, inside mask 1010
    0x04, 0x0B, 0x29, 0xFF, 0xFF, 0xFF,      // tetrahedron 1, inside mask 1011
    0x04, 0x0D, 0x0B, 0x04, 0x06, 0x0D,      // tetrahedron 1, inside mask 1100
    0x00, 0x0D, 0x0B, 0xFF, 0xFF, 0xFF,      // tetrahedron 1, inside mask 1101
    0x00, 0x04, 0x06, 0xFF, 0xFF, 0xFF,      // tetrahedron 1, inside mask 1110
    0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,      // tetrahedron 1, inside mask 1111
    0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,      // tetrahedron 2, inside mask 0000
    0x01, 0x06, 0x02, 0xFF, 0xFF, 0xFF,      // tetrahedron 2, inside mask 0001
    0x01, 0x10, 0x14, 0xFF, 0xFF, 0xFF,      // tetrahedron 2, inside mask 0010
    0x02, 0x14, 0x06, 0x02, 0x10, 0x14,      // tetrahedron 2, inside mask 0011
    0x02, 0x1B, 0x10, 0xFF, 0xFF, 0xFF,      // tetrahedron 2, inside mask 0100
    0x01, 0x06, 0x1B, 0x01, 0x1B, 0x10,      // tetrahedron 2, inside mask 0101
    0x01, 0x1B, 0x14, 0x01, 0x02, 0x1B,      // tetrahedron 2, inside mask 0110
    0x06, 0x1B, 0x14, 0xFF, 0xFF, 0xFF,      // tetrahedron 2, inside mask 0111
    0x06, 0x14, 0x1B, 0xFF, 0xFF, 0xFF,      // tetrahedron 2, inside mask 1000
    0x01, 0x1B, 0x02, 0x01, 0x14, 0x1B,      // tetrahedron 2, inside mask 1001
    0x01, 0x10, 0x1B, 0x01, 0x1B, 0x06,      // tetrahedron 2, inside mask 1010
    0x02, 0x10, 0x1B, 0xFF, 0xFF, 0xFF,      // tetrahedron 2, inside mask 1011
    0x02, 0x14, 0x10, 0x02, 0x06, 0x14,      // tetrahedron 2, inside mask 1100
    0x01, 0x14, 0x10, 0xFF, 0xFF, 0xFF,      // tetrahedron 2, inside mask 1101
    0x01, 0x02, 0x06, 0xFF, 0xFF, 0xFF,      // tetrahedron 2, inside mask 1110
    0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,      // tetrahedron 2, inside mask 1111
    0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,      // tetrahedron 3, inside mask 0000
    0x01, 0x05, 0x06, 0xFF, 0xFF, 0xFF,      // tetrahedron 3, inside mask 0001
    0x01, 0x14, 0x13, 0xFF, 0xFF, 0xFF,      // tetrahedron 3, inside mask 0010
    0x05, 0x06, 0x14, 0x05, 0x14, 0x13,      // tetrahedron 3, inside mask 0011
    0x05, 0x13, 0x30, 0xFF, 0xFF, 0xFF,      // tetrahedron 3, inside mask 0100
    0x01, 0x30, 0x06, 0x01, 0x13, 0x30,      // tetrahedron 3, inside mask 0101
    0x01, 0x14, 0x30, 0x01, 0x30, 0x05,      // tetrahedron 3, inside mask 0110
    0x06, 0x14, 0x30, 0xFF, 0xFF, 0xFF,      // tetrahedron 3, inside mask 0111
    0x06, 0x30, 0x14, 0xFF, 0xFF, 0xFF,      // tetrahedron 3, inside mask 1000
    0x01, 0x05, 0x30, 0x01, 0x30, 0x14,      // tetrahedron 3, inside mask 1001
    0x01, 0x30, 0x13, 0x01, 0x06, 0x30,      // tetrahedron 3, inside mask 1010
    0x05, 0x30, 0x13, 0xFF, 0xFF, 0xFF,      // tetrahedron 3, inside mask 1011
    0x05, 0x13, 0x14, 0x05, 0x14, 0x06,      // tetrahedron 3, inside mask 1100
    0x01, 0x13, 0x14, 0xFF, 0xFF, 0xFF,      // tetrahedron 3, inside mask 1101
    0x01, 0x06, 0x05, 0xFF, 0xFF, 0xFF,      // tetrahedron 3, inside mask 1110
    0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,      // tetrahedron 3, inside mask 1111
    0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,      // tetrahedron 4, inside mask 0000
    0x03, 0x04, 0x06, 0xFF, 0xFF, 0xFF,      // tetrahedron 4, inside mask 0001
    0x03, 0x22, 0x20, 0xFF, 0xFF, 0xFF,      // tetrahedron 4, inside mask 0010
    0x04, 0x06, 0x22, 0x04, 0x22, 0x20,      // tetrahedron 4, inside mask 0011
    0x04, 0x20, 0x29, 0xFF, 0xFF, 0xFF,      // tetrahedron 4, inside mask 0100
    0x03, 0x29, 0x06, 0x03, 0x20, 0x29,      // tetrahedron 4, inside mask 0101
    0x03, 0x22, 0x29, 0x03, 0x29, 0x04,      // tetrahedron 4, inside mask 0110
    0x06, 0x22, 0x29, 0xFF, 0xFF, 0xFF,      // tetrahedron 4, inside mask 0111
    0x06, 0x29, 0x22, 0xFF, 0xFF, 0xFF,      // tetrahedron 4, inside mask 1000
    0x03, 0x04, 0x29, 0x03, 0x29, 0x22,      // tetrahedron 4, inside mask 1001
    0x03, 0x29, 0x20, 0x03, 0x06, 0x29,      // tetrahedron 4, inside mask 1010
    0x04, 0x29, 0x20, 0xFF, 0xFF, 0xFF,      // tetrahedron 4, inside mask 1011
    0x04, 0x20, 0x22, 0x04, 0x22, 0x06,      // tetrahedron 4, inside mask 1100
    0x03, 0x20, 0x22, 0xFF, 0xFF, 0xFF,      // tetrahedron 4, inside mask 1101
    0x03, 0x06, 0x04, 0xFF, 0xFF, 0xFF,      // tetrahedron 4, inside mask 1110
    0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,      // tetrahedron 4, inside mask 1111
    0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,      // tetrahedron 5, inside mask 0000
    0x03, 0x06, 0x05, 0xFF, 0xFF, 0xFF,      // tetrahedron 5, inside mask 0001
    0x03, 0x21, 0x22, 0xFF, 0xFF, 0xFF,      // tetrahedron 5, inside mask 0010
    0x05, 0x22, 0x06, 0x05, 0x21, 0x22,      // tetrahedron 5, inside mask 0011
    0x05, 0x30, 0x21, 0xFF, 0xFF, 0xFF,      // tetrahedron 5, inside mask 0100
    0x03, 0x06, 0x30, 0x03, 0x30, 0x21,      // tetrahedron 5, inside mask 0101
    0x03, 0x30, 0x22, 0x03, 0x05, 0x30,      // tetrahedron 5, inside mask 0110
    0x06, 0x30, 0x22, 0xFF, 0xFF, 0xFF,      // tetrahedron 5, inside mask 0111
    0x06, 0x22, 0x30, 0xFF, 0xFF, 0xFF,      // tetrahedron 5, inside mask 1000
    0x03, 0x30, 0x05, 0x03, 0x22, 0x30,      // tetrahedron 5, inside mask 1001
    0x03, 0x21, 0x30, 0x03, 0x30, 0x06,      // tetrahedron 5, inside mask 1010
    0x05, 0x21, 0x30, 0xFF, 0xFF, 0xFF,      // tetrahedron 5, inside mask 1011
    0x05, 0x22, 0x21, 0x05, 0x06, 0x22,      // tetrahedron 5, inside mask 1100
    0x03, 0x22, 0x21, 0xFF, 0xFF, 0xFF,      // tetrahedron 5, inside mask 1101
    0x03, 0x05, 0x06, 0xFF, 0xFF, 0xFF,      // tetrahedron 5, inside mask 1110
    0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,      // tetrahedron 5, inside mask 1111
};

__device__ __forceinline__ int tet_mask(unsigned corners, int t) {
    return (corners & 1) | (((corners >> kTetMid[t][0]) & 1) << 1) | (((corners >> kTetMid[t][1]) & 1) << 2) |
           (((corners >> 7) & 1) << 3);
}

// Inside bits of the eight corners of cube (x, y, z), bit c = corner c; x < nx - 1.
__device__ __forceinline__ unsigned cube_corners(const float *__restrict__ field, int nx, int ny, int x, int y, int z,
                                                 float level) {
    unsigned bits = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const size_t p = ((size_t)(z + (c >> 2)) * ny + (y + ((c >> 1) & 1))) * nx + (x + (c & 1));
        bits |= (field[p] > level ? 1u : 0u) << c;
    }
    return bits;
}

__device__ __forceinline__ int cube_triangles(unsigned corners) {
    int n = 0;
#pragma unroll
    for (int t = 0; t < kMeshTets; t++) {
        const int in = __popc(tet_mask(corners, t));
        n += in == 2 ? 2 : ((in == 1 || in == 3) ? 1 : 0);
    }
    return n;
}

__global__ __launch_bounds__(kBatchThreads) void mesh_count_kernel(const float *__restrict__ field, int nx, int ny,
                                                                  float level, int32_t *__restrict__ row_count) {
    __shared__ int red[kBatchWaves];
    const int row = blockIdx.x, y = row % (ny - 1), z = row / (ny - 1);
    int n = 0;
    for (int x0 = 0; x0 < nx - 1; x0 += kBatchThreads) {
        const int x = x0 + threadIdx.x;
        if (x < nx - 1) n += cube_triangles(cube_corners(field, nx, ny, x, y, z, level));
    }
    const int total = block_sum(n, red);
    if (threadIdx.x == 0) row_count[row] = total;
}

__global__ __launch_bounds__(kBatchThreads) void mesh_emit_kernel(const float *__restrict__ field, int nx, int ny,
                                                                 float level, const int64_t *__restrict__ row_start,
                                                                 int64_t T, int64_t *__restrict__ tri_keys) {
    __shared__ int red[kBatchWaves];
    __shared__ uint8_t table[kMeshTableBytes];
    for (int i = threadIdx.x; i < kMeshTableBytes; i += kBatchThreads) table[i] = kCaseTable[i];
    __syncthreads();
    const int row = blockIdx.x, y = row % (ny - 1), z = row / (ny - 1);
    int64_t base = row_start[row];
    for (int x0 = 0; x0 < nx - 1; x0 += kBatchThreads) {
        const int x = x0 + threadIdx.x;
        const unsigned corners = x < nx - 1 ? cube_corners(field, nx, ny, x, y, z, level) : 0u;
        int chunk;
        int64_t out = base + block_excl_scan(cube_triangles(corners), red, chunk);      // (no corner inside: no triangle)
        base += chunk;
        const int64_t lo = ((int64_t)z * ny + y) * nx + x;
#pragma unroll
        for (int t = 0; t < kMeshTets; t++) {
            const uint8_t *e = table + (t * 16 + tet_mask(corners, t)) * 6;
#pragma unroll
            for (int k = 0; k < 2; k++) {
                if (e[3 * k] == kMeshEmpty) continue;
                if (out < T) {                         // out < T: a caller's T below the scan's total cannot write past the end
#pragma unroll
                    for (int v = 0; v < 3; v++) {
                        const int code = e[3 * k + v], c = code >> 3;
                        const int64_t p = lo + (c & 1) + (int64_t)((c >> 1) & 1) * nx + (int64_t)(c >> 2) * nx * ny;
                        tri_keys[out * 3 + v] = p * 7 + (code & 7);
                    }
                }
                out++;
            }
        }
    }
}

__global__ __launch_bounds__(kBatchThreads) void mesh_vertices_kernel(const int64_t *__restrict__ keys, int64_t V,
                                                                     const float *__restrict__ field, int nx, int ny, int nz,
                                                                     float level, double min_x, double min_y, double min_z,
                                                                     double h, float *__restrict__ pos) {
    const int64_t i = (int64_t)blockIdx.x * kBatchThreads + threadIdx.x;
    if (i >= V) return;
    const int64_t key = keys[i], lo = key / 7;
    const int kind = (int)(key - lo * 7) + 1;
    const int dx = kind & 1, dy = (kind >> 1) & 1, dz = kind >> 2;
    const int64_t plane = (int64_t)nx * ny;
    const int z = (int)(lo / plane), y = (int)((lo - z * plane) / nx), x = (int)(lo - z * plane - (int64_t)y * nx);
    if (key < 0 || z + dz >= nz || y + dy >= ny || x + dx >= nx) {      // a key that names no edge of this grid
        pos[i * 3 + 0] = pos[i * 3 + 1] = pos[i * 3 + 2] = __builtin_nanf("");
        return;
    }
    const double fa = (double)field[lo], fb = (double)field[lo + dx + (int64_t)dy * nx + dz * plane];
    double t = __ddiv_rn(__dsub_rn((double)level, fa), __dsub_rn(fb, fa));
    if (!(t >= 0.0 && t <= 1.0)) t = 0.5;              // only non-finite end values give such a t
    const double px = __dadd_rn((double)x, __dmul_rn(t, (double)dx));
    const double py = __dadd_rn((double)y, __dmul_rn(t, (double)dy));
    const double pz = __dadd_rn((double)z, __dmul_rn(t, (double)dz));
    pos[i * 3 + 0] = (float)__dadd_rn(min_x, __dmul_rn(px, h));
    pos[i * 3 + 1] = (float)__dadd_rn(min_y, __dmul_rn(py, h));
    pos[i * 3 + 2] = (float)__dadd_rn(min_z, __dmul_rn(pz, h));
}

static bool mesh_grid_ok(int32_t nx, int32_t ny, int32_t nz) {
    return nx >= 2 && ny >= 2 && nz >= 2 && (int64_t)nx * ny * nz < (1ll << 31);
}

}  // namespace occ

OCC_API int occnerf_mesh_count(const float *field, int32_t nx, int32_t ny, int32_t nz, float level, int32_t *row_count,
                               void *stream) {
    using namespace occ;
    OCC_REQUIRE(field && row_count, "mesh_count: null argument");
    OCC_REQUIRE(mesh_grid_ok(nx, ny, nz), "mesh_count: bad grid %d x %d x %d (every axis >= 2 points, fewer than 2^31 in all)",
                nx, ny, nz);
    hipLaunchKernelGGL(mesh_count_kernel, dim3((nz - 1) * (ny - 1)), dim3(kBatchThreads), 0, as_stream(stream), field, nx, ny,
                       level, row_count);
    return check_launch("mesh_count");
}

OCC_API int occnerf_mesh_emit(const float *field, int32_t nx, int32_t ny, int32_t nz, float level, const int64_t *row_start,
                              int64_t T, int64_t *tri_keys, void *stream) {
    using namespace occ;
    OCC_REQUIRE(field && row_start, "mesh_emit: null argument");
    OCC_REQUIRE(mesh_grid_ok(nx, ny, nz), "mesh_emit: bad grid %d x %d x %d (every axis >= 2 points, fewer than 2^31 in all)",
                nx, ny, nz);
    OCC_REQUIRE(T >= 0, "mesh_emit: T=%lld is negative", (long long)T);
    if (T == 0) return 0;
    OCC_REQUIRE(tri_keys, "mesh_emit: null tri_keys with T=%lld", (long long)T);
    hipLaunchKernelGGL(mesh_emit_kernel, dim3((nz - 1) * (ny - 1)), dim3(kBatchThreads), 0, as_stream(stream), field, nx, ny,
                       level, row_start, T, tri_keys);
    return check_launch("mesh_emit");
}

OCC_API int occnerf_mesh_vertices(const int64_t *keys, int64_t V, const float *field, int32_t nx, int32_t ny, int32_t nz,
                                  float level, const double *h_bbox_min, double h, float *pos, void *stream) {
    using namespace occ;
    OCC_REQUIRE(field && h_bbox_min, "mesh_vertices: null argument");
    OCC_REQUIRE(mesh_grid_ok(nx, ny, nz), "mesh_vertices: bad grid %d x %d x %d (every axis >= 2 points, fewer than 2^31 in all)",
                nx, ny, nz);
    OCC_REQUIRE(V >= 0 && V < 7 * (1ll << 31), "mesh_vertices: V=%lld outside [0, 7 * 2^31)", (long long)V);
    if (V == 0) return 0;
    OCC_REQUIRE(keys && pos, "mesh_vertices: null keys / pos with V=%lld", (long long)V);
    hipLaunchKernelGGL(mesh_vertices_kernel, dim3((unsigned)((V + kBatchThreads - 1) / kBatchThreads)), dim3(kBatchThreads), 0,
                       as_stream(stream), keys, V, field, nx, ny, nz, level, h_bbox_min[0], h_bbox_min[1], h_bbox_min[2], h, pos);
    return check_launch("mesh_vertices");
}
