// The training batch of a prepared dataset frame, built on the device (reference core/data/occnerf/train.py:167-273
// get_patch_ray_indices / _get_patch_ray_indices, :322-348 sample_patch_rays, :296-297 + :398 the blend).  The frame's image
// and mask stay resident as uint8; occnerf_gen_rays has written the ray of every pixel and the box mask.  Three launches:
//   1. classify   one workgroup per image row: how many pixels of the row are subject (mask channel 0 > 0, train.py:470)
//                 and how many are off-subject (box hit and not subject, :179-182);
//   2. pick       one workgroup per patch: the class from u0, the k-th set pixel of the class in row-major order
//                 (np.where's order, :236-242) from u1 by a scan over the row counts and a scan inside the row, then the
//                 clipped top-left corner (:245-253).  Integer work only;
//   3. gather     one workgroup per patch: ordered compaction of the patch pixels whose ray hits the box (wave64 ballots
//                 and popcounts, one LDS scan across the waves, chunks of 256 pixels so any patch size loops), the rows'
//                 rays / near / far / target colour, the whole patch's blended target, its mask and the two row <-> pixel
//                 maps.  A patch's first row is the number of box pixels of the patches before it, which every workgroup
//                 recounts (at most N * S * S byte loads) instead of waiting for its neighbours.
// No atomics, no host wait; every output is a pure function of the inputs.
//
// The blend is the reference's float64 expression, one rounding per operator (the tree is built with -ffp-contract=off):
//   ((m / 255.) * image + (1.0 - m / 255.) * bgcolor) / 255.  -> float32.
#include "batch_common.h"

namespace occ {

constexpr int kMaxPatches = 64;

struct PatchDraws {
    double u[kMaxPatches][2];
};

// class 0: subject, class 1: box and not subject
template <class Pixels>
__device__ __forceinline__ bool in_class(const Pixels &px, const uint8_t *__restrict__ box, int p, int cls) {
    const bool subject = px.subject((size_t)p);
    return cls == 0 ? subject : (box[p] != 0 && !subject);
}

// Pixels: where the frame's pixels are read from, PixelsU8 or PixelsF64 (batch_common.h)
template <class Pixels>
__global__ __launch_bounds__(kBatchThreads) void batch_classify_kernel(const Pixels px, const uint8_t *__restrict__ box,
                                                                      int H, int W, int32_t *__restrict__ row_counts) {
    __shared__ int red[kBatchWaves];
    const int row = blockIdx.x;
    int n0 = 0, n1 = 0;
    for (int x0 = 0; x0 < W; x0 += kBatchThreads) {
        const int x = x0 + threadIdx.x;
        bool s = false, o = false;
        if (x < W) {
            const int p = row * W + x;
            s = px.subject((size_t)p);
            o = box[p] != 0 && !s;
        }
        n0 += __popcll(__ballot(s));                   // wave-uniform
        n1 += __popcll(__ballot(o));
    }
    const bool lead = (threadIdx.x & (kWave - 1)) == 0;
    const int t0 = block_sum(lead ? n0 : 0, red);
    const int t1 = block_sum(lead ? n1 : 0, red);
    if (threadIdx.x == 0) {
        row_counts[row] = t0;
        row_counts[H + row] = t1;
    }
}

template <class Pixels>
__global__ __launch_bounds__(kBatchThreads) void batch_pick_kernel(const Pixels px, const uint8_t *__restrict__ box, int H,
                                                                  int W, int size,
                                                                  PatchDraws draws, double subject_ratio,
                                                                  const int32_t *__restrict__ row_counts,
                                                                  int32_t *__restrict__ xy_min) {
    __shared__ int red[kBatchWaves];
    __shared__ int found[2];                           // row, index inside the row; then centre x
    const int patch = blockIdx.x, t = threadIdx.x;
    const int per = (H + kBatchThreads - 1) / kBatchThreads;
    const int r0 = min(t * per, H), r1 = min(r0 + per, H);
    int s0 = 0, s1 = 0;
    for (int r = r0; r < r1; r++) {
        s0 += row_counts[r];
        s1 += row_counts[H + r];
    }
    int total0, total1;
    const int e0 = block_excl_scan(s0, red, total0);
    const int e1 = block_excl_scan(s1, red, total1);
    int cls = draws.u[patch][0] < subject_ratio ? 0 : 1;                 // train.py:195
    if ((cls == 0 ? total0 : total1) == 0) cls ^= 1;                     // empty class: the other one (documented fallback)
    const int count = cls == 0 ? total0 : total1;
    int cx = 0, cy = 0;
    if (count > 0) {                                                     // wave- and block-uniform
        long long k = (long long)floor(draws.u[patch][1] * (double)count);
        k = k < 0 ? 0 : (k > count - 1 ? count - 1 : k);
        const int excl = cls == 0 ? e0 : e1, mine = cls == 0 ? s0 : s1;
        if (k >= excl && k < excl + mine) {                              // exactly one thread
            int rem = (int)k - excl;
            for (int r = r0; r < r1; r++) {
                const int c = row_counts[cls * H + r];
                if (rem < c) {
                    found[0] = r;
                    found[1] = rem;
                    break;
                }
                rem -= c;
            }
        }
        __syncthreads();
        cy = found[0];
        const int rem_row = found[1];
        const int perw = (W + kBatchThreads - 1) / kBatchThreads;
        const int x0 = min(t * perw, W), x1 = min(x0 + perw, W);
        int sw = 0;
        for (int x = x0; x < x1; x++) sw += in_class(px, box, cy * W + x, cls) ? 1 : 0;
        int totalw;
        const int ew = block_excl_scan(sw, red, totalw);
        if (rem_row >= ew && rem_row < ew + sw) {
            int rem = rem_row - ew;
            for (int x = x0; x < x1; x++) {
                if (in_class(px, box, cy * W + x, cls)) {
                    if (rem == 0) {
                        found[0] = x;
                        break;
                    }
                    rem--;
                }
            }
        }
        __syncthreads();
        cx = found[0];
    }
    if (t == 0) {
        const int half = size / 2;                                       // train.py:245-253
        xy_min[patch * 2 + 0] = min(max(cx - half, 0), W - size);
        xy_min[patch * 2 + 1] = min(max(cy - half, 0), H - size);
    }
}

struct BatchOut {
    float *rays, *near, *far, *target_rgbs, *target_patches;
    uint8_t *patch_masks;
    int32_t *patch_div_indices, *pix_of_row, *row_of_pix, *n_rows;
};

template <class Pixels>
__global__ __launch_bounds__(kBatchThreads) void batch_gather_kernel(const Pixels px, const float *__restrict__ rays8,
                                                                    const uint8_t *__restrict__ box, int W, int n_patches,
                                                                    int size, double bg0, double bg1, double bg2,
                                                                    const int32_t *__restrict__ xy_min, BatchOut out) {
    __shared__ int red[kBatchWaves];
    const int patch = blockIdx.x, t = threadIdx.x;
    const int npix = size * size;
    const int64_t rmax = (int64_t)n_patches * npix;
    // first row of this patch: the box pixels of the patches drawn before it
    int before = 0;
    for (int q = 0; q < patch; q++) {
        const int qx = xy_min[q * 2], qy = xy_min[q * 2 + 1];
        for (int i = t; i < npix; i += kBatchThreads) before += box[(qy + i / size) * W + qx + i % size] != 0 ? 1 : 0;
    }
    int base = block_sum(before, red);
    if (t == 0) out.patch_div_indices[patch] = base;
    const int x_min = xy_min[patch * 2], y_min = xy_min[patch * 2 + 1];
    const double bg[3] = {bg0, bg1, bg2};
    for (int i0 = 0; i0 < npix; i0 += kBatchThreads) {
        const int i = i0 + t;
        const bool live = i < npix;
        const int p = live ? (y_min + i / size) * W + x_min + i % size : 0;
        const bool hit = live && box[p] != 0;
        int chunk;
        const int row = base + chunk_rank(hit, red, chunk);
        base += chunk;
        if (!live) continue;
        const int64_t pix = (int64_t)patch * npix + i;
        float rgb[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {                  // train.py:296-297, :398 in float64, one rounding per operator
            rgb[c] = px.target((size_t)p, c, bg[c]);
            out.target_patches[pix * 3 + c] = rgb[c];
        }
        out.patch_masks[pix] = hit ? 1 : 0;
        out.row_of_pix[pix] = hit ? row : -1;
        if (hit) {
            store_ray_row(rays8 + (size_t)p * 8, row, rmax, out.rays, out.near, out.far);
#pragma unroll
            for (int c = 0; c < 3; c++) out.target_rgbs[(int64_t)row * 3 + c] = rgb[c];
            out.pix_of_row[row] = (int32_t)pix;
        }
    }
    if (patch == n_patches - 1 && t == 0) {
        out.patch_div_indices[n_patches] = base;
        out.n_rows[0] = base;
    }
}

// The three launches from either pixel source; `first` and `second` are its two pointers, checked with the rest.
template <class Pixels>
static int patch_batch_from(const Pixels px, const void *first, const void *second, const float *rays8,
                            const uint8_t *box_mask, int32_t H, int32_t W, int32_t n_patches, int32_t size, const double *h_u,
                            double subject_ratio, const float *h_bgcolor, int32_t *row_counts, float *rays, float *near,
                            float *far, float *target_rgbs, float *target_patches, uint8_t *patch_masks,
                            int32_t *patch_div_indices, int32_t *xy_min, int32_t *pix_of_row, int32_t *row_of_pix,
                            int32_t *n_rows, void *stream) {
    OCC_REQUIRE(first && second && rays8 && box_mask && h_u && h_bgcolor && row_counts && rays && near && far && target_rgbs &&
                    target_patches && patch_masks && patch_div_indices && xy_min && pix_of_row && row_of_pix && n_rows,
                "patch_batch: null argument");
    OCC_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < (1ll << 28), "patch_batch: bad image size %d x %d", H, W);
    OCC_REQUIRE(n_patches >= 1 && n_patches <= kMaxPatches, "patch_batch: n_patches=%d outside [1, %d]", n_patches, kMaxPatches);
    OCC_REQUIRE(size >= 1 && size <= H && size <= W, "patch_batch: patch size %d does not fit a %d x %d image", size, H, W);
    PatchDraws draws;
    for (int p = 0; p < n_patches; p++) {
        draws.u[p][0] = h_u[p * 2];
        draws.u[p][1] = h_u[p * 2 + 1];
        OCC_REQUIRE(draws.u[p][0] >= 0.0 && draws.u[p][0] < 1.0 && draws.u[p][1] >= 0.0 && draws.u[p][1] < 1.0,
                    "patch_batch: the uniforms of patch %d are not in [0, 1)", p);
    }
    for (int p = n_patches; p < kMaxPatches; p++) draws.u[p][0] = draws.u[p][1] = 0.0;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(batch_classify_kernel<Pixels>, dim3(H), dim3(kBatchThreads), 0, st, px, box_mask, H, W, row_counts);
    hipLaunchKernelGGL(batch_pick_kernel<Pixels>, dim3(n_patches), dim3(kBatchThreads), 0, st, px, box_mask, H, W, size, draws,
                       subject_ratio, (const int32_t *)row_counts, xy_min);
    BatchOut out{rays, near, far, target_rgbs, target_patches, patch_masks, patch_div_indices, pix_of_row, row_of_pix, n_rows};
    hipLaunchKernelGGL(batch_gather_kernel<Pixels>, dim3(n_patches), dim3(kBatchThreads), 0, st, px, rays8, box_mask, W,
                       n_patches, size, (double)h_bgcolor[0], (double)h_bgcolor[1], (double)h_bgcolor[2],
                       (const int32_t *)xy_min, out);
    return check_launch("patch_batch");
}

}  // namespace occ

OCC_API int32_t occnerf_patch_batch_max_patches(void) { return occ::kMaxPatches; }

OCC_API int occnerf_patch_batch(const uint8_t *image, const uint8_t *alpha, const float *rays8, const uint8_t *box_mask,
                                int32_t H, int32_t W, int32_t n_patches, int32_t size, const double *h_u,
                                double subject_ratio, const float *h_bgcolor, int32_t *row_counts, float *rays, float *near,
                                float *far, float *target_rgbs, float *target_patches, uint8_t *patch_masks,
                                int32_t *patch_div_indices, int32_t *xy_min, int32_t *pix_of_row, int32_t *row_of_pix,
                                int32_t *n_rows, void *stream) {
    return occ::patch_batch_from(occ::PixelsU8{image, alpha}, image, alpha, rays8, box_mask, H, W, n_patches, size, h_u,
                                 subject_ratio, h_bgcolor, row_counts, rays, near, far, target_rgbs, target_patches,
                                 patch_masks, patch_div_indices, xy_min, pix_of_row, row_of_pix, n_rows, stream);
}

OCC_API int occnerf_patch_batch_f64(const double *img64, const double *alpha64, const float *rays8, const uint8_t *box_mask,
                                    int32_t H, int32_t W, int32_t n_patches, int32_t size, const double *h_u,
                                    double subject_ratio, const float *h_bgcolor, int32_t *row_counts, float *rays,
                                    float *near, float *far, float *target_rgbs, float *target_patches, uint8_t *patch_masks,
                                    int32_t *patch_div_indices, int32_t *xy_min, int32_t *pix_of_row, int32_t *row_of_pix,
                                    int32_t *n_rows, void *stream) {
    return occ::patch_batch_from(occ::PixelsF64{img64, alpha64}, img64, alpha64, rays8, box_mask, H, W, n_patches, size, h_u,
                                 subject_ratio, h_bgcolor, row_counts, rays, near, far, target_rgbs, target_patches,
                                 patch_masks, patch_div_indices, xy_min, pix_of_row, row_of_pix, n_rows, stream);
}
