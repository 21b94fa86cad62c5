// Connected components of a welded triangle mesh (occnerf_amd/mesh.py component_table): two triangles
// are connected when they share a vertex index; the label of a component is the smallest vertex index in it.
//   occnerf_mesh_label_pass       one pass over labels[V] (the caller starts them at labels[v] = v): a hook launch, one thread
//                                 per triangle, then a compress launch, one thread per vertex.  The host repeats passes until
//                                 one changes nothing (ops.mesh_label);
//   occnerf_mesh_component_stats  the integer record of every component: one thread per vertex (vertices, boundary vertices,
//                                 the snapped box), one per triangle (triangles, six times the snapped signed volume).
// Why passes and no single-kernel union-find: every store to labels[] only ever LOWERS a word (atomicMin, or the compress
// launch's store of a smaller value by the word's only writer) and labels[v] <= v holds throughout, so a plain load that
// returns an older value -- this CU's L1, another XCD's L2 -- names a vertex of the same component that is no smaller than the
// current one: it delays convergence, it cannot make a label wrong.  Nothing waits on another workgroup.  A pass whose atomics
// all returned a value they did not lower changed no word, so every load of that pass saw the values the kernel boundary
// made coherent: the host's stopping test reads a state that is a true fixed point.
// The records are integer sums, minima and maxima: any order of the atomics gives the same bits.  The body takes nearly all
// of them, so each wave first reduces over its runs of equal component rank (vertices come in key order, triangles in
// emission order: a run is usually the whole wave) and the head lane of a run issues the atomics.
#include "batch_common.h"

namespace occ {

constexpr double kSnapScale = 1024.0;                  // snapped coordinates: 1/1024 of a voxel edge
constexpr double kSnapLimit = 1073741824.0;            // |s| <= 2^30: an int32 whatever the input holds

// Hook: m = the smallest of the three labels goes into the three vertices and into the three vertices those labels name (their
// trees' tops, as far as this thread can see), so two trees that meet in a triangle merge in one pass instead of one hop per
// pass.  m <= la <= a, so labels[x] <= x is kept; atomicMin only lowers.  status[0] |= 1 when an atomic lowered a word,
// status[1] = 1 when a face names a vertex outside [0, V) (nothing of that face is touched).
__global__ __launch_bounds__(kBatchThreads) void mesh_hook_kernel(const int32_t *__restrict__ faces, int64_t T, int64_t V,
                                                                 int32_t *labels, int32_t *status) {
    const int64_t t = (int64_t)blockIdx.x * kBatchThreads + threadIdx.x;
    if (t >= T) return;
    const int32_t a = faces[t * 3 + 0], b = faces[t * 3 + 1], c = faces[t * 3 + 2];
    if (a < 0 || b < 0 || c < 0 || a >= V || b >= V || c >= V) {
        status[1] = 1;
        return;
    }
    const int32_t la = labels[a], lb = labels[b], lc = labels[c];
    if (la < 0 || lb < 0 || lc < 0 || la > a || lb > b || lc > c) {      // not labels this entry made: refuse, follow nothing
        status[1] = 1;
        return;
    }
    const int32_t m = min(la, min(lb, lc));
    bool changed = false;
    // (a word already read as m needs no atomic: if that read was stale the word is lower still)
    if (la != m) changed |= atomicMin(labels + a, m) > m;
    if (lb != m) changed |= atomicMin(labels + b, m) > m;
    if (lc != m) changed |= atomicMin(labels + c, m) > m;
    if (la != m) changed |= atomicMin(labels + la, m) > m;
    if (lb != m) changed |= atomicMin(labels + lb, m) > m;
    if (lc != m) changed |= atomicMin(labels + lc, m) > m;
    if (changed) status[0] = 1;
}

// Compress: labels[v] = the top of v's chain.  The loop is finite by construction: it goes on only while labels[r] < r, so r
// strictly decreases and is bounded by 0; a value outside [0, r) ends it.  Thread v is the only writer of labels[v] in this
// launch and writes a value no larger than the one it read.
__global__ __launch_bounds__(kBatchThreads) void mesh_compress_kernel(int64_t V, int32_t *labels, int32_t *status) {
    const int64_t v = (int64_t)blockIdx.x * kBatchThreads + threadIdx.x;
    if (v >= V) return;
    const int32_t first = labels[v];
    if (first < 0 || first > v) {
        status[1] = 1;
        return;
    }
    int32_t r = first;
    for (;;) {
        const int32_t p = labels[r];
        if (p < 0 || p >= r) break;
        r = p;
    }
    if (r != first) {
        labels[v] = r;
        status[0] = 1;
    }
}

// llrint(((float64(x) - lo) / h) * 1024), one rounding per operator, held to [-2^30, 2^30] (a NaN goes to the lower end).
__device__ __forceinline__ int32_t snap(float x, double lo, double h) {
    double q = __dmul_rn(__ddiv_rn(__dsub_rn((double)x, lo), h), kSnapScale);
    if (!(q >= -kSnapLimit)) q = -kSnapLimit;
    if (q > kSnapLimit) q = kSnapLimit;
    return (int32_t)llrint(q);
}

// The number of this lane's run within the wave: lanes are in one run while their keys are equal and consecutive.
__device__ __forceinline__ int run_of_lane(int32_t key, bool &head) {
    const int lane = threadIdx.x & (kWave - 1);
    const int32_t before = __shfl_up(key, 1);
    head = lane == 0 || before != key;
    const unsigned long long heads = __ballot(head);
    return __popcll(heads & ((2ull << lane) - 1ull));                  // heads at or below this lane
}

// Segmented reductions over the runs of a wave (run numbers ascend with the lane, so an equal number `o` lanes up means the
// lanes between belong to the run too); the head lane of each run ends with the run's result.
template <typename T, typename Op>
__device__ __forceinline__ T run_reduce(T v, int run, Op op) {
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const T other = __shfl_down(v, o);
        const int other_run = __shfl_down(run, o);
        if (lane + o < kWave && other_run == run) v = op(v, other);
    }
    return v;
}

struct OpAdd {
    template <typename T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct OpMin {
    __device__ __forceinline__ int32_t operator()(int32_t a, int32_t b) const { return a < b ? a : b; }
};
struct OpMax {
    __device__ __forceinline__ int32_t operator()(int32_t a, int32_t b) const { return a > b ? a : b; }
};

// counts[C,3]: vertices, triangles, boundary vertices; box[C,6]: smin, smax.  A lane past V, or one whose rank is outside
// [0, C), has the key -1 and adds nothing.
__global__ __launch_bounds__(kBatchThreads) void mesh_vertex_stats_kernel(const float *__restrict__ verts, int64_t V,
                                                                         const int32_t *__restrict__ vrank, int64_t C,
                                                                         double min_x, double min_y, double min_z, double h,
                                                                         int32_t ex, int32_t ey, int32_t ez,
                                                                         int32_t *counts, int32_t *box) {
    const int64_t v = (int64_t)blockIdx.x * kBatchThreads + threadIdx.x;
    int32_t key = -1, s[3] = {0, 0, 0}, on_boundary = 0;
    if (v < V) {
        const int32_t r = vrank[v];
        if (r >= 0 && r < C) key = r;
        s[0] = snap(verts[v * 3 + 0], min_x, h);
        s[1] = snap(verts[v * 3 + 1], min_y, h);
        s[2] = snap(verts[v * 3 + 2], min_z, h);
        on_boundary = (s[0] == 0 || s[0] == ex || s[1] == 0 || s[1] == ey || s[2] == 0 || s[2] == ez) ? 1 : 0;
    }
    bool head;
    const int run = run_of_lane(key, head);
    const int32_t n = run_reduce<int32_t>(key >= 0 ? 1 : 0, run, OpAdd());
    const int32_t nb = run_reduce<int32_t>(on_boundary, run, OpAdd());
    int32_t lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = run_reduce<int32_t>(s[a], run, OpMin());
        hi[a] = run_reduce<int32_t>(s[a], run, OpMax());
    }
    if (!head || key < 0) return;
    atomicAdd(counts + (int64_t)key * 3 + 0, n);
    if (nb) atomicAdd(counts + (int64_t)key * 3 + 2, nb);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        atomicMin(box + (int64_t)key * 6 + a, lo[a]);
        atomicMax(box + (int64_t)key * 6 + 3 + a, hi[a]);
    }
}

// vol6[C] += det(s_a, s_b, s_c) = a_x (b_y c_z - b_z c_y) + a_y (b_z c_x - b_x c_z) + a_z (b_x c_y - b_y c_x) in 64-bit
// two's-complement arithmetic with wrap-around (unsigned here: the same bits, and no signed overflow in the source).  The
// triangle belongs to the component of its first vertex.  A face that names a vertex outside [0, V) adds nothing.
__global__ __launch_bounds__(kBatchThreads) void mesh_triangle_stats_kernel(const float *__restrict__ verts, int64_t V,
                                                                           const int32_t *__restrict__ faces, int64_t T,
                                                                           const int32_t *__restrict__ vrank, int64_t C,
                                                                           double min_x, double min_y, double min_z, double h,
                                                                           int32_t *counts, unsigned long long *vol6) {
    const int64_t t = (int64_t)blockIdx.x * kBatchThreads + threadIdx.x;
    int32_t key = -1;
    unsigned long long det = 0;
    if (t < T) {
        const int32_t i[3] = {faces[t * 3 + 0], faces[t * 3 + 1], faces[t * 3 + 2]};
        if (i[0] >= 0 && i[1] >= 0 && i[2] >= 0 && i[0] < V && i[1] < V && i[2] < V) {
            const int32_t r = vrank[i[0]];
            if (r >= 0 && r < C) key = r;
            unsigned long long s[3][3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                s[k][0] = (unsigned long long)(long long)snap(verts[(int64_t)i[k] * 3 + 0], min_x, h);
                s[k][1] = (unsigned long long)(long long)snap(verts[(int64_t)i[k] * 3 + 1], min_y, h);
                s[k][2] = (unsigned long long)(long long)snap(verts[(int64_t)i[k] * 3 + 2], min_z, h);
            }
            det = s[0][0] * (s[1][1] * s[2][2] - s[1][2] * s[2][1]) + s[0][1] * (s[1][2] * s[2][0] - s[1][0] * s[2][2]) +
                  s[0][2] * (s[1][0] * s[2][1] - s[1][1] * s[2][0]);
        }
    }
    if (key < 0) det = 0;
    bool head;
    const int run = run_of_lane(key, head);
    const int32_t n = run_reduce<int32_t>(key >= 0 ? 1 : 0, run, OpAdd());
    const unsigned long long sum = run_reduce<unsigned long long>(det, run, OpAdd());
    if (!head || key < 0) return;
    atomicAdd(counts + (int64_t)key * 3 + 1, n);
    if (sum) atomicAdd(vol6 + key, sum);
}

static unsigned mesh_blocks(int64_t n) { return (unsigned)((n + kBatchThreads - 1) / kBatchThreads); }

}  // namespace occ

OCC_API int occnerf_mesh_label_pass(const int32_t *faces, int64_t T, int64_t V, int32_t *labels, int32_t *status,
                                    void *stream) {
    using namespace occ;
    OCC_REQUIRE(T >= 0 && T < (1ll << 31) && V >= 0 && V < (1ll << 31), "mesh_label_pass: T=%lld / V=%lld outside [0, 2^31)",
                (long long)T, (long long)V);
    OCC_REQUIRE(status, "mesh_label_pass: null status");
    if (V == 0) return 0;
    OCC_REQUIRE(labels && (faces || T == 0), "mesh_label_pass: null labels / faces with V=%lld, T=%lld", (long long)V,
                (long long)T);
    if (T > 0) {
        hipLaunchKernelGGL(mesh_hook_kernel, dim3(mesh_blocks(T)), dim3(kBatchThreads), 0, as_stream(stream), faces, T, V,
                           labels, status);
        if (int rc = check_launch("mesh_label_pass (hook)")) return rc;
    }
    hipLaunchKernelGGL(mesh_compress_kernel, dim3(mesh_blocks(V)), dim3(kBatchThreads), 0, as_stream(stream), V, labels,
                       status);
    return check_launch("mesh_label_pass (compress)");
}

OCC_API int occnerf_mesh_component_stats(const float *verts, int64_t V, const int32_t *faces, int64_t T, const int32_t *vrank,
                                         int64_t C, const double *h_bbox_min, double h, int32_t nx, int32_t ny, int32_t nz,
                                         int32_t *counts, int32_t *box, int64_t *vol6, void *stream) {
    using namespace occ;
    OCC_REQUIRE(T >= 0 && T < (1ll << 31) && V >= 0 && V < (1ll << 31), "mesh_component_stats: T=%lld / V=%lld outside [0, 2^31)",
                (long long)T, (long long)V);
    OCC_REQUIRE(C >= 0 && C <= V, "mesh_component_stats: C=%lld outside [0, V=%lld]", (long long)C, (long long)V);
    OCC_REQUIRE(h_bbox_min, "mesh_component_stats: null h_bbox_min");
    OCC_REQUIRE(h > 0.0 && h <= 1.7976931348623157e308, "mesh_component_stats: h=%g must be a positive finite number", h);
    OCC_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2 && nx <= (1 << 20) && ny <= (1 << 20) && nz <= (1 << 20),
                "mesh_component_stats: bad grid %d x %d x %d (every axis 2 .. 2^20 points)", nx, ny, nz);
    if (V == 0 || C == 0) return 0;
    OCC_REQUIRE(verts && vrank && counts && box && vol6 && (faces || T == 0), "mesh_component_stats: null argument with V=%lld",
                (long long)V);
    hipLaunchKernelGGL(mesh_vertex_stats_kernel, dim3(mesh_blocks(V)), dim3(kBatchThreads), 0, as_stream(stream), verts, V,
                       vrank, C, h_bbox_min[0], h_bbox_min[1], h_bbox_min[2], h, (nx - 1) * 1024, (ny - 1) * 1024,
                       (nz - 1) * 1024, counts, box);
    if (int rc = check_launch("mesh_component_stats (vertices)")) return rc;
    if (T > 0) {
        hipLaunchKernelGGL(mesh_triangle_stats_kernel, dim3(mesh_blocks(T)), dim3(kBatchThreads), 0, as_stream(stream), verts, V,
                           faces, T, vrank, C, h_bbox_min[0], h_bbox_min[1], h_bbox_min[2], h, counts,
                           reinterpret_cast<unsigned long long *>(vol6));
        return check_launch("mesh_component_stats (triangles)");
    }
    return 0;
}
