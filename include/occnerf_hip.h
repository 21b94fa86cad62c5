/*
 * occnerf_hip.h -- C ABI of the MI355X (gfx950) implementation of OccNeRF's per-ray
 * volumetric rendering hot path.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name starts with h_ (host);
 *   - caller owns all buffers, outputs are caller-allocated (the reference's FFI
 *     convention, gridencoder/src/gridencoder.cu:448-503);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); launches are
 *     asynchronous, nothing here synchronises;
 *   - return value: 0 on success, non-zero on error (invalid argument or a HIP error);
 *     occnerf_last_error() returns a thread-local description.  The Python host layer
 *     turns a non-zero return into RuntimeError, matching the reference's TORCH_CHECK
 *     -> c10::Error -> RuntimeError behaviour (gridencoder.cu:15-18).
 *
 * Section 1 is the reference's own native operator interface for this path (the
 * `_gridencoder` pybind module).  Section 2 are the fused stages that sit behind the
 * reference's *module* seam (core/nets/occnerf/network.py `Network`,
 * canonical_mlps/occnerf_mlp.py `CanonicalMLP`): the reference evaluates them as chains
 * of torch ops and has no FFI for them; each entry cites the Python it replaces.  The
 * last entries serve the reference's scripts around the renderer: LPIPS for training, the
 * patch images, and eval.py's per-frame metrics (SSIM / PSNR / IoU, which the reference
 * takes from skimage and numpy on the host).
 */
#ifndef OCCNERF_HIP_H
#define OCCNERF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an existing export's signature or a table layout changes (2: composite/msknn_clustered/
 * sample_features grew arguments in round 2, the Adam table row carries per-tensor bias corrections; 3: msknn_clustered
 * takes the cluster groups; 4: occnerf_agg_backward takes a scratch buffer; 5: round 6 -- the experiment knobs cohab_lds,
 * features_small, features_rowcache, linear_resident and split_refill and the kernels behind them left the library; the two
 * f16x3 calls take a domain flag). */
#define OCCNERF_ABI_VERSION 5

int occnerf_abi_version(void);
const char *occnerf_last_error(void);

/* Tuning knobs.  Two remain, both choosing between shipped forms with identical results: "agg_slices" (OCCNERF_AGG_SLICES,
 * 0 = automatic, else the sample slices of occnerf_agg_backward) and "grid_xcd" (OCCNERF_GRID_XCD: the operator-level D4C2
 * forward with the level pairs dealt to the XCDs -- 0: from 32 768 samples up (the default), 1: always, 2: never;
 * profiles/r05_xcd_levels.md).  Each is read from its environment variable once, at first use, and clamped to its valid range;
 * this call reads (value < 0) or sets it afterwards.  Returns the previous value, -1 for an unknown name.  No launch in this
 * library alters its outputs for diagnosis.  No counterpart in the reference. */
int occnerf_experiment_knob(const char *name, int value);

/* ------------------------------------------------------------------------------------
 * 1. Grid encoder -- replaces core/nets/occnerf/gridencoder/src/bindings.cpp:5-9
 *    (prototypes gridencoder.h:12-15, kernels gridencoder.cu:87-369,506-645).
 *    Argument order and meaning are the reference's; at::Tensor -> pointer, and the
 *    trailing stream is new (the reference launches on the legacy default stream).
 *    D in {2,3,4,5}, C in {1,2,4,8}.  The reference dispatches on the tensors' dtype
 *    (AT_DISPATCH_FLOATING_TYPES_AND_HALF, gridencoder.cu:467,500); a C ABI has no tensor to
 *    ask, so the dtype is in the entry point's name: no suffix = float32 (what the rendering
 *    path uses), _f16 = at::Half (what grid.py:44-45 feeds under autocast), _f64 = double.
 * ---------------------------------------------------------------------------------- */

/* inputs[B,D] in [0,1] (rows outside -> zeros); embeddings[sO,C]; offsets[L+1] int32;
 * outputs[L,B,C] written in place; dy_dx[B,L*D*C] or NULL.
 * S = log2(per_level_scale), H = base resolution, gridtype 0 hash / 1 tiled,
 * interp 0 linear / 1 smoothstep.                         gridencoder.cu:448-471 */
int occnerf_grid_encode_forward(const float *inputs, const float *embeddings,
                                const int32_t *offsets, float *outputs, uint32_t B, uint32_t D,
                                uint32_t C, uint32_t L, float S, uint32_t H, float *dy_dx,
                                uint32_t gridtype, int align_corners, uint32_t interp,
                                void *stream);

/* grad[L,B,C]; grad_embeddings[sO,C] must be zero-filled by the caller and is
 * accumulated with fp32 atomics; dy_dx / grad_inputs[B,D] optional (both or neither).
 *                                                          gridencoder.cu:473-503 */
int occnerf_grid_encode_backward(const float *grad, const float *inputs, const float *embeddings,
                                 const int32_t *offsets, float *grad_embeddings, uint32_t B,
                                 uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                 const float *dy_dx, float *grad_inputs, uint32_t gridtype,
                                 int align_corners, uint32_t interp, void *stream);

/* occnerf_grid_encode_forward with the level offsets also given as a HOST array h_offsets[L+1]: the D = 4, C = 2 hash
 * encoder without dy_dx (what the canonical MLP evaluates on every sample) then runs as 8 lanes per sample x 2 levels
 * per lane with the per-level index mode (dense / power-of-two mask / generic) decided on the host; identical
 * results.  Everything else falls through to the reference-shaped kernel. */
int occnerf_grid_encode_forward_h(const float *inputs, const float *embeddings, const int32_t *offsets,
                                  const int32_t *h_offsets, float *outputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                  float S, uint32_t H, float *dy_dx, uint32_t gridtype, int align_corners,
                                  uint32_t interp, void *stream);

/* Host-side helper of the module's backward (grid.py:69-90 permutes autograd's [B, L*C] gradient to [L,B,C] before the
 * operator call): the same transposition with the rows of RUNS of consecutive samples whose inputs are bitwise identical
 * summed into the run's first sample, zeros in the others (the tiled backward skips zero rows).  Same gradient (another
 * summation order); only when no input gradient is wanted.  No counterpart in the reference. */
int occnerf_grid_grad_runs(const float *grad_rows, const float *inputs, int64_t B, uint32_t D, uint32_t L, uint32_t C,
                           float *grad, void *stream);

/* occnerf_grid_encode_backward with the level offsets also given as a HOST array h_offsets[L+1].  The
 * reference's signature above cannot know the level sizes without reading device memory, so it always runs
 * the atomic scatter (gridencoder.cu:248-340 as written); with the host copy, large D = 4, C = 2 hash batches
 * take the atomics-free path (workgroup-owned LDS tiles of the table, fp64 accumulators).  scratch (optional, device,
 * scratch_bytes >= L * B * 8): room for the per-(level, sample) tile sets of the pre-pass that lets a tile-job hash only the
 * samples that touch it; without it every tile-job re-hashes every sample (same results). */
int occnerf_grid_encode_backward_h(const float *grad, const float *inputs, const float *embeddings,
                                   const int32_t *offsets, const int32_t *h_offsets, float *grad_embeddings,
                                   uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                   const float *dy_dx, float *grad_inputs, uint32_t gridtype, int align_corners,
                                   uint32_t interp, void *scratch, int64_t scratch_bytes, void *stream);

/* The at::Half dispatch case of the two operators above (gridencoder.cu:467,500).  embeddings, outputs, dy_dx, grad,
 * grad_embeddings, grad_inputs are IEEE binary16 arrays (torch.half); inputs stay float32, as in the reference
 * (`const float *inputs`, gridencoder.cu:373).  Arithmetic follows c10::Half exactly: cell position and corner weights in
 * float, every `scalar_t +=` a half-rounded term added in float and rounded to half (GridMath<half_t> in
 * occnerf_amd/csrc/grid_encode.hip spells it out); the backward adds channel pairs with packed-half atomics
 * (gridencoder.cu:323-331), so C must be even there -- the reference's own C = 1 half path is an empty stub (:22-26) and grid.py:44 never selects it. */
int occnerf_grid_encode_forward_f16(const float *inputs, const void *embeddings, const int32_t *offsets, void *outputs,
                                    uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, void *dy_dx,
                                    uint32_t gridtype, int align_corners, uint32_t interp, void *stream);
int occnerf_grid_encode_backward_f16(const void *grad, const float *inputs, const void *embeddings, const int32_t *offsets,
                                     void *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                     uint32_t H, const void *dy_dx, void *grad_inputs, uint32_t gridtype, int align_corners,
                                     uint32_t interp, void *stream);

/* The double dispatch case (gridencoder.cu:467,500 with scalar_t = double): embeddings, outputs, dy_dx, grad, grad_embeddings,
 * grad_inputs are float64; inputs stay float32 and so do the cell position, the corner weights and pos_deriv, exactly as the
 * reference's templates leave them; products with the double tensors are formed in double and `r += a * b` is one fma
 * (GridMath<double> in csrc/grid_encode.hip).  The backward scatters with global_atomic_add_f64.  With the two calls above
 * this completes AT_DISPATCH_FLOATING_TYPES_AND_HALF: no dtype the reference's `_gridencoder` accepts is refused. */
int occnerf_grid_encode_forward_f64(const float *inputs, const double *embeddings, const int32_t *offsets, double *outputs,
                                    uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, double *dy_dx,
                                    uint32_t gridtype, int align_corners, uint32_t interp, void *stream);
int occnerf_grid_encode_backward_f64(const double *grad, const float *inputs, const double *embeddings, const int32_t *offsets,
                                     double *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                     uint32_t H, const double *dy_dx, double *grad_inputs, uint32_t gridtype, int align_corners,
                                     uint32_t interp, void *stream);

/* Total-variation gradient, gridencoder.cu:506-645.  Never called by the reference's
 * trainer; exported for interface completeness and
 * returns an error ("not implemented") without touching its arguments. */
int occnerf_grad_total_variation(const float *inputs, const float *embeddings, float *grad,
                                 const int32_t *offsets, float weight, uint32_t B, uint32_t D,
                                 uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                 int align_corners, void *stream);

/* ------------------------------------------------------------------------------------
 * 2. Sample pipeline (behind Network.forward / CanonicalMLP.forward)
 * ---------------------------------------------------------------------------------- */

/* Ray sampling + backward warp to canonical space.
 * Replaces network.py:405-432 (_unpack_ray_batch, _get_samples_along_ray,
 * _stratified_sampling), :456 (pts) and :351-402 (_sample_motion_fields).
 * rays[n,8] = (o, d, near, far); t_vals[S] = linspace(0,1,S); t_rand[n,S] or NULL;
 * Rs[nb,3,3], Ts[nb,3]: motion bases; vol[>=nb,G,G,G]: motion-weight volume (a trailing
 * background channel is ignored); h_bbox_min[3], h_bbox_scale[3] on the HOST.
 * Outputs z_vals[n,S], x_skel[n*S,3], mask[n*S]; pts[n*S,3] optional (NULL to skip). */
int occnerf_sample_warp(const float *rays, int64_t n, int32_t S, const float *t_vals,
                        const float *t_rand, const float *Rs, const float *Ts, const float *vol,
                        int32_t nb, int32_t G, const float *h_bbox_min, const float *h_bbox_scale,
                        float *z_vals, float *pts, float *x_skel, float *mask, void *stream);
/* The renderer's form (no jitter, no pts): same outputs, bit for bit, with the bones whose motion-weight channel cannot
 * reach a wave's 64 samples skipped.  boxes[nb,6] int32 = {x0,x1,y0,y1,z0,z1} of every channel's non-zero voxels, from
 * occnerf_bone_boxes on the same vol (x0 > x1: all zero).  The culling applies when S is a multiple of 64 (a wave's samples
 * then lie on one ray); otherwise the call behaves like occnerf_sample_warp. */
int occnerf_bone_boxes(const float *vol, int32_t nb, int32_t G, int32_t *boxes, void *stream);
int occnerf_sample_warp_culled(const float *rays, int64_t n, int32_t S, const float *t_vals,
                               const float *Rs, const float *Ts, const float *vol, int32_t nb, int32_t G,
                               const int32_t *boxes, const float *h_bbox_min, const float *h_bbox_scale,
                               float *z_vals, float *x_skel, float *mask, void *stream);

/* Render order of a frame's rays: the permutation that walks them along a 2-D Morton curve of their directions (projected on
 * the plane normal to the mean direction), so that 64 consecutive rays are a compact ~8x8 pixel patch (kNN tiles, hash-grid
 * gathers) and 256 a ~16x16 one (the block a rank is dealt).  No counterpart in the reference, whose ray order is the
 * dataset's (freeview.py:190-208 row-major pixels); rays are independent, results are returned in the caller's order.
 * dirs: R directions `stride` floats apart (3: a [R,3] array; 8: columns 3..5 of rays8); order[R] int64 out; temp:
 * occnerf_ray_order_temp_bytes(R) bytes.  Deterministic (fixed-order reductions + a stable radix sort): every rank of a
 * sharded render computes the same walk from the same frame. */
int64_t occnerf_ray_order_temp_bytes(int64_t R);
int occnerf_ray_order(const float *dirs, int64_t R, int64_t stride, int64_t *order, void *temp, int64_t temp_bytes,
                      void *stream);

/* Per-frame ray generation (one thread per pixel): camera_util.py:133-160 get_rays_from_KRT +
 * :163-212 rays_intersect_3d_bbox, as the reference's datasets call them (tpose.py:155-172,
 * freeview.py:190-208).  HOST inputs: h_Kinv[9] = K^-1, h_R[9], h_T[3] (E[:3,:3], E[:3,3]), row major,
 * h_bbox_min/max[3] = the observation-space skeleton bbox (the 0.01 growth is applied inside);
 * f32_camera != 0: K and E were float32 arrays, so numpy ran pixel -> ray in float32 (the reference's
 * synthetic tpose / freeview cameras); 0: float64 (calibrated dataset cameras).
 * Outputs for every pixel p = row * W + col: rays8[p] = (origin, direction with |d|<1e-5 clamped as the
 * reference clamps it, near, far) and mask[p] = 1 when the ray crosses the box (exactly two face hits);
 * near/far are 0 where mask is 0.  The caller compacts by mask (occnerf_amd/rays.py). */
int occnerf_gen_rays(const double *h_Kinv, const double *h_R, const double *h_T, int32_t f32_camera,
                     int32_t H, int32_t W, const double *h_bbox_min, const double *h_bbox_max, float *rays8,
                     uint8_t *mask, void *stream);

/* Non-rigid offset MLP (105 -> 128 x6 (skip @4) -> 3) with the Hann-windowed Fourier
 * embedding.  Replaces embedders/hannw_fourier.py:9-63 + mlp_offset.py:45-62 as called at
 * network.py:225-232.
 * occnerf_nonrigid_pack: h_W/h_b = HOST arrays of the 7 device weight/bias pointers
 * (block_mlps.{0,2,...,12}, torch layout) -> packed[occnerf_nonrigid_packed_floats()], once
 * per checkpoint.  occnerf_nonrigid: cond[69] is the frame's condition code (folded into the
 * layer-0 bias inside `packed`, which is therefore written per call), W0/b0 the layer-0
 * weight/bias, h_hann[6] the HOST window weights.  xyz_out may alias xyz_in. */
int64_t occnerf_nonrigid_packed_floats(void);
int occnerf_nonrigid_pack(const float *const *h_W, const float *const *h_b, float *packed,
                          void *stream);
int occnerf_nonrigid(const float *xyz_in, int64_t N, const float *cond, const float *h_hann,
                     const float *W0, const float *b0, float *packed, float *xyz_out,
                     void *stream);
/* occnerf_nonrigid, in place, on the samples rows[0 .. *n_dev) of xyz[N_max,3] only (the frame's live samples;
 * list and count in device memory, occnerf_live_rows). */
int occnerf_nonrigid_rows(float *xyz, int64_t N_max, const int32_t *rows, const int32_t *n_dev,
                          const float *cond, const float *h_hann, const float *W0, const float *b0,
                          float *packed, void *stream);
/* The first fp32 version (32-sample waves, weights straight from L2); same arguments and packed buffer,
 * same results to fp32 rounding.  Cross-check and A/B timing; occnerf_nonrigid is the LDS-staged
 * 16-sample-tile kernel. */
int occnerf_nonrigid_direct(const float *xyz_in, int64_t N, const float *cond, const float *h_hann,
                            const float *W0, const float *b0, float *packed, float *xyz_out,
                            void *stream);

/* bf16x3 variant of the non-rigid MLP (split-bf16 operands, fp32 accumulation; see
 * occnerf_canonical_mlp_bf16x3).  packed = the fp32 blob (biases, folded layer-0 bias, output
 * rows); packed_bf16 = occnerf_nonrigid_packed_bf16_bytes() zero-initialised bytes filled by
 * occnerf_nonrigid_pack_bf16 from the first 6 weight pointers. */
int64_t occnerf_nonrigid_packed_bf16_bytes(void);
int occnerf_nonrigid_pack_bf16(const float *const *h_W, void *packed_bf16, void *stream);
int occnerf_nonrigid_bf16x3(const float *xyz_in, int64_t N, const float *cond, const float *h_hann,
                            const float *W0, const float *b0, float *packed, const void *packed_bf16,
                            float *xyz_out, void *stream);
/* In place on the listed samples only (as occnerf_nonrigid_rows for the fp32 kernel): xyz[rows[i]] += offset for
 * i < *n_dev (device-side count, <= N_max). */
int occnerf_nonrigid_bf16x3_rows(float *xyz, int64_t N_max, const int32_t *rows, const int32_t *n_dev,
                                 const float *cond, const float *h_hann, const float *W0, const float *b0,
                                 float *packed, const void *packed_bf16, void *stream);

/* Multi-scale exact kNN (k = 10, up to 4 point sets).  Replaces the pykeops
 * Kmin_argKmin reduction of knn.py:77-85 and the index bookkeeping of network.py:235-255.
 * points[M,3]: the scales concatenated (scale 0 = all base points first);
 * h_scale_begin[nscale+1] host prefix offsets into points; index_map[M]: base-point index
 * of every row (identity for scale 0, fps_index for the others);
 * h_seed_from_coarser[nscale]: non-zero when scale s is a superset of scale s+1, which lets
 * the search bound its radius by the coarser result (results are identical either way).
 * knn_idxs[N,nscale,10] int32, ascending distance, ties -> lower row first. */
int occnerf_msknn(const float *xyz, int64_t N, const float *points, const int32_t *index_map,
                  const int32_t *h_scale_begin, const int32_t *h_seed_from_coarser,
                  int32_t nscale, int32_t *knn_idxs, void *stream);

/* The same search with cluster culling (same results, ~5x fewer distance evaluations on the
 * SMPL body).  Queries are xyz[n_rays * samples_per_ray, 3] in ray-major order; a wavefront
 * works on 64 consecutive rays x 4 consecutive samples (callers that order rays in compact pixel
 * patches get the most out of it; any order is correct) and skips every cluster of support
 * points that the triangle inequality puts outside all of its queries' search radii.
 * Layout (built by the host once per model, occnerf_amd/geometry.py::build_knn_clusters):
 * points[M,4] = every scale but the coarsest stored cluster by cluster (cluster = nearest
 * coarsest-scale point), then the coarsest scale in original order at rows
 * h_coarse_rows[0..1); segments padded to multiples of 4 rows with +inf points; .w (int bits) =
 * original row within the scale << 16 | base-point index: the row is the tie-break key among equal
 * distances, the base index (< 65536) is what knn_idxs reports; centers[ncl,4];
 * cluster_ranges[nscale-1,ncl,2] row ranges into points; cluster_radius[nscale-1,ncl] >=
 * max |p - center| per cluster.  group_centers[ngrp,4], group_ranges[ngrp,2], group_radius[nscale-1,ngrp] (nullable together,
 * ngrp = 0): the clusters are listed group by group -- group g = clusters group_ranges[g][0..1) -- and group_radius bounds
 * everything those clusters hold at a scale around group_centers[g] (< 0: nothing there), so a search tests the group spheres
 * first and only the clusters of the groups in reach; same results.  mask (nullable) [n_rays * samples_per_ray]: samples whose mask is
 * exactly 0 (motion-weight sum, network.py:330: their alpha is multiplied by it) are skipped and their
 * knn_idxs rows left unwritten.  query_rows / n_query_dev / ray_start (nullable, together, instead of mask): the ascending
 * list of the samples to query (occnerf_live_rows or the heads of occnerf_repeat_heads) with its length in device memory and
 * an int32[n_rays + 1] scratch; a lane then takes the next four LISTED samples of its ray instead of four fixed sample slots,
 * so tiles are full wherever their rays still have listed samples. */
int occnerf_msknn_clustered(const float *xyz, const float *mask, int64_t n_rays, int32_t samples_per_ray,
                            const float *points, const float *centers,
                            const int32_t *cluster_ranges, const float *cluster_radius, int32_t ncl,
                            const float *group_centers, const int32_t *group_ranges, const float *group_radius, int32_t ngrp,
                            const int32_t *h_coarse_rows, const int32_t *h_seed_from_coarser,
                            int32_t nscale, const int32_t *query_rows, const int32_t *n_query_dev, int32_t *ray_start,
                            int32_t *knn_idxs, void *stream);
/* Centre cache.  occnerf_knn_center searches ONE point c[3] (device memory) against the brute-force layout of occnerf_msknn
 * (points[M,4], index_map[M], h_scale_begin[nscale+1]) and writes center_out[4] = (c, r^2) and idx_out[nscale,10]: c's neighbours
 * and the squared radius inside which every query provably has the same neighbours in the same order (0: none, e.g. a tie among
 * c's 11 nearest).  occnerf_msknn_clustered_centered is occnerf_msknn_clustered with that pair (nullable together): queries with
 * |q - c|^2 < r^2 receive idx_out without a search, tiles that hold no other query are skipped.  Same knn_idxs, bit for bit.
 * The renderer passes c = the non-rigid offset of the origin, onto which the samples with a vanishing motion-weight sum
 * collapse (two thirds of the live samples of a frame). */
int occnerf_knn_center(const float *c, const float *points, const int32_t *index_map, const int32_t *h_scale_begin,
                       int32_t nscale, float *center_out, int32_t *idx_out, void *stream);
int occnerf_msknn_clustered_centered(const float *xyz, const float *mask, int64_t n_rays, int32_t samples_per_ray,
                                     const float *points, const float *centers,
                                     const int32_t *cluster_ranges, const float *cluster_radius, int32_t ncl,
                                     const float *group_centers, const int32_t *group_ranges, const float *group_radius, int32_t ngrp,
                                     const int32_t *h_coarse_rows, const int32_t *h_seed_from_coarser,
                                     int32_t nscale, const int32_t *query_rows, const int32_t *n_query_dev, int32_t *ray_start,
                                     const float *center, const int32_t *center_idx, int32_t *knn_idxs, void *stream);

/* Plain exact kNN for small problems (k <= 16): idx[nq,k] rows of s, ascending.
 * Used for the per-point k=3 search of network.py:265-269 and the k=10 visibility update
 * of network.py:508-512. */
int occnerf_knn_small(const float *q, int32_t nq, const float *s, int32_t ns, int32_t k,
                      int32_t *idx, void *stream);

/* unit[P,3] = normals / max(|normals|, 1e-8) in float64: the normal-side half of
 * F.cosine_similarity (network.py:275, occnerf_mlp.py:165).  A per-model constant, computed
 * once after generate_neural_points and passed to the two functions below. */
int occnerf_unit_normals(const double *normals, int32_t P, double *unit, void *stream);

/* Per-point signed-distance block, network.py:263-284 (chunk-invariant; once per frame).
 * point_cloud[P,3] = point_base + point_dist; normals[P,3] float64; kidx[P,3] from
 * occnerf_knn_small.  Outputs knn_base[P,3] float64, dist[P] fp32. */
int occnerf_point_sdf(const float *point_cloud, const float *point_base, const double *normals,
                      const double *unit_normals, const int32_t *kidx, int32_t P,
                      double *knn_base, float *dist, void *stream);

/* Per-point feature table, occnerf_mlp.py:171-175:
 * table[P,T], T = occnerf_point_table_stride() floats (64: 256-byte rows, so that the 128-byte encoding
 * part of a gathered row is exactly one cache line); columns
 *   [encode((knn_base+bound)/(2 bound), clamp((sdf+0.2)/0.8,0,1)) (32), learnable xyz (3), 0, unused...].
 * h_offsets: optional HOST copy of offsets[L+1]; with it the kernel knows per level whether the
 * table is dense or a power-of-two hash and skips the generic 32-bit modulo (same indices). */
/* Training step: gradient of the learnable point offsets point_dist[P] (network.py:109,119: point_cloud = point_base +
 * point_dist, one offset per point added to all three coordinates) through occnerf_point_sdf -- network.py:263-284 under
 * autograd -- from d_knn_base[P,3] (fp64) and d_dist[P]; kidx: the 3-NN ids of the forward (constants of the graph). */
int occnerf_point_sdf_backward(const float *point_cloud, const float *point_base, const double *normals,
                               const double *unit_normals, const int32_t *kidx, int32_t P, const double *d_knn_base,
                               const float *d_dist, float *d_point_dist, void *stream);
int32_t occnerf_point_table_stride(void);
int occnerf_point_table(const double *knn_base, const float *point_sdf, const float *learnable,
                        int32_t P, float bound, float two_bound, const float *embeddings,
                        const int32_t *offsets, const int32_t *h_offsets, uint32_t L, float S,
                        uint32_t H, float *table, void *stream);

/* Per-sample features: neighbour geometry + hash encoding + visibility-softmax
 * aggregation.  Replaces occnerf_mlp.py:144-181 (+ simple_agg :86-126).
 * knn_idxs[N,nscale,10]: base-point rows; counter[P] visibility counts; table from
 * occnerf_point_table.  Outputs mlp_in[N,68] = [agg(35), var(1), enc(32)] and raw[N,5]
 * column 4 (signed distance); enc_in[N,4] optional (NULL to skip).
 * Two optional inputs serve callers that hold the reference's *gathered* CanonicalMLP
 * arguments instead of per-point arrays: geo_idxs[N,10] (rows of point_base/normals to use
 * for the geometry prelude instead of knn_idxs[:,0,:]) and att_in[N,nscale*10] (visibility
 * counts already gathered, used instead of counter[knn_idxs]); NULL for the normal path.
 * rows (nullable, renderer's path only): a compact list of N sample indices into xyz / knn_idxs -- the
 * samples that can contribute to their pixel (motion-weight sum != 0); output row m then belongs to
 * sample rows[m].  n_dev (nullable, needs rows): the length of the list in device memory; N is then the
 * capacity of the outputs.
 * point_geo[P,16] / point_tail[P,4] (nullable, together; from occnerf_point_pack): the per-point inputs repacked so that
 * one gather brings everything the prelude / the softmax needs of a point; with them (and 4 scales, no gathered
 * inputs) the 8-lanes-per-sample kernel runs, without them the thread-per-sample one (same results bit for bit).
 * P: rows of point_geo / point_tail (ignored without them). */
int occnerf_point_pack(const float *point_base, const double *normals, const double *unit_normals,
                       const float *counter, const float *table, int32_t P, float *point_geo,
                       float *point_tail, void *stream);
int occnerf_sample_features(const float *xyz, int64_t N, const int32_t *knn_idxs, int32_t nscale,
                            const float *point_base, const double *normals,
                            const double *unit_normals, const float *counter,
                            const float *table, float bound, float two_bound,
                            const float *embeddings, const int32_t *offsets,
                            const int32_t *h_offsets, uint32_t L, float S, uint32_t H,
                            const int32_t *geo_idxs, const float *att_in, const int32_t *rows,
                            const int32_t *n_dev, const float *point_geo, const float *point_tail, int32_t P,
                            float *mlp_in, float *raw, float *enc_in, void *stream);
/* The renderer's form with the kNN centre cache (occnerf_knn_center): center[4] = (c, r^2) and center_agg[72] = of a sample that
 * has c's neighbour lists (this function on a sample at c) columns 0..35 of mlp_in, the encoder input x[4] (enc_in), columns
 * 36..67 of mlp_in.  A group of 8 consecutive listed samples that all lie inside the radius -- they all carry c's 40 ids --
 * copies columns 0..35 instead of gathering the 40 rows, and columns 36..67 as well when every one of its encoder inputs equals
 * the centre's bit for bit.  Same outputs, bit for bit.  Both pointers nullable together. */
int occnerf_sample_features_centered(const float *xyz, int64_t N, const int32_t *knn_idxs, int32_t nscale,
                            const float *point_base, const double *normals,
                            const double *unit_normals, const float *counter,
                            const float *table, float bound, float two_bound,
                            const float *embeddings, const int32_t *offsets,
                            const int32_t *h_offsets, uint32_t L, float S, uint32_t H,
                            const int32_t *geo_idxs, const float *att_in, const int32_t *rows,
                            const int32_t *n_dev, const float *point_geo, const float *point_tail, int32_t P,
                            const float *center, const float *center_agg,
                                     float *mlp_in, float *raw, float *enc_in, void *stream);

/* Differentiable neighbour aggregation of the training path (occnerf_mlp.py:86-126 simple_agg with the
 * gather of :176-178): agg[n,:] = sum_j atts[n,j] * feats[knn[n,j],:] for feats[P,F] (F <= 64), knn[N,K],
 * atts[N,K] (detached in the reference).  Backward: partial[W,P,F] with W = occnerf_agg_backward_slices(N);
 * every element is written, grad_feats = partial.sum(0).  Workgroups own (sample slice, point tile) pairs
 * and accumulate in LDS -- no global atomics; a first pass sums the gradient rows of runs of consecutive samples with
 * bitwise identical neighbour lists AND weights (K <= 64; arbitrary atts are exact: round 6 compares them too) into `scratch`
 * (occnerf_agg_backward_scratch_bytes(N, F) bytes) so that a run is scattered once.  Limits, refused by name: F <= 64, K <= 64 in
 * the backward, and at most 32 point tiles (P <= 32 x min(1024, 18432 / F) rows: 16 832 at F = 35).  Replaces torch's feats[knn]
 * materialisation and its index_put backward. */
int occnerf_agg_forward(const float *feats, int32_t F, const int32_t *knn, const float *atts, int64_t N, int32_t K,
                        float *agg, void *stream);
int32_t occnerf_agg_backward_slices(int64_t N);
int64_t occnerf_agg_backward_scratch_bytes(int64_t N, int32_t F);
int occnerf_agg_backward(const float *grad_agg, int32_t F, const int32_t *knn, const float *atts, int64_t N,
                         int32_t K, int32_t P, float *partial, void *scratch, int64_t scratch_bytes, void *stream);

/* Live samples of a frame (mask = per-sample motion-weight sum, network.py:330: alpha is multiplied by it).
 * rows[0 .. *count) = ascending indices of the samples with mask != 0, both in device memory; temp = device
 * scratch of occnerf_live_rows_temp_bytes(N) bytes.  occnerf_scatter_raw copies the compact raw_c[m, 0..4] rows
 * to raw_full[rows[m], 0..4] for m < *n_dev (raw_full zero-initialised by the caller). */
int64_t occnerf_live_rows_temp_bytes(int64_t N);
int occnerf_live_rows(const float *mask, int64_t N, int32_t *rows, int32_t *count, void *temp,
                      int64_t temp_bytes, void *stream);
int occnerf_scatter_raw(const float *raw_c, const int32_t *rows, const int32_t *n_dev, int64_t N_max,
                        float *raw_full, void *stream);

/* Repeated samples.  Every stage after the warp is a pure per-sample function (occnerf_mlp.py:144-199, mlp_offset.py:45-62),
 * and consecutive entries of a frame's sample list often carry bitwise identical inputs (where the motion-weight sum is far
 * below the clamp of network.py:324 the warped position collapses onto the origin).  occnerf_repeat_heads compares the key
 * of entry m -- key_dwords 32-bit words at keys + r * stride_dwords, r = rows ? rows[m] : m -- with entry m-1's as bit
 * patterns for m < *n_dev and writes scan[m] = number of entries 0..m that differ from their predecessor ("heads"; entry 0
 * is one), heads[scan[m]-1] = r for every head, *head_count, and, when head_mask is given (zero-filled by the caller),
 * head_mask[r] = 1.  scan has N_max entries (those beyond *n_dev repeat the total); temp = device scratch of
 * occnerf_repeat_heads_temp_bytes(N_max) bytes.  occnerf_scatter_raw_heads: raw_full[rows[m], 0..3] = raw_h[h, 0..3] and
 * raw_full[rows[m], 4] = raw_c[a, 4] with a = scanA ? scanA[m]-1 : m and h = scanB ? scanB[a]-1 : a.
 * occnerf_canonical_mlp_rows: occnerf_canonical_mlp_counted reading input row in_rows[n] for output row n. */
int64_t occnerf_repeat_heads_temp_bytes(int64_t N_max);
int occnerf_repeat_heads(const void *keys, int64_t stride_dwords, int32_t key_dwords, const int32_t *rows,
                         const int32_t *n_dev, int64_t N_max, int32_t *scan, int32_t *heads, int32_t *head_count,
                         float *head_mask, void *temp, int64_t temp_bytes, void *stream);
/* Distinct entries of a whole list (what run-length elimination leaves: equal keys that are not neighbours).  Entry j < *n_dev
 * is row r = heads ? heads[j] : j with the key of occnerf_repeat_heads; entries are grouped by an open-addressing table
 * (atomicCAS on a slot, full-key compare against the claimant), heads_out / *count_out list one representative row per
 * distinct key in ascending entry order, and scan (nullable, with its device-side length and capacity) -- a map whose
 * values are 1-based entry numbers, e.g. occnerf_repeat_heads' scan -- is rewritten to 1-based positions in heads_out.  Which
 * of several equal entries represents them is not deterministic; since their keys are equal bit for bit, results are.
 * temp = device scratch of occnerf_unique_heads_temp_bytes(cap) bytes; cap = capacity of the list. */
int64_t occnerf_unique_heads_temp_bytes(int64_t cap);
int occnerf_unique_heads(const void *keys, int64_t stride_dwords, int32_t key_dwords, const int32_t *heads,
                         const int32_t *n_dev, int64_t cap, int32_t *heads_out, int32_t *count_out, int32_t *scan,
                         const int32_t *n_scan_dev, int64_t scan_cap, void *temp, int64_t temp_bytes, void *stream);
int occnerf_scatter_raw_heads(const float *raw_h, const float *raw_c, const int32_t *rows, const int32_t *n_dev,
                              const int32_t *scanA, const int32_t *scanB, int64_t N_max, float *raw_full, void *stream);
int occnerf_canonical_mlp_rows(const float *mlp_in, const int32_t *in_rows, int64_t N_max, const int32_t *n_dev,
                               const float *packed, float *raw, void *stream);

/* Canonical MLP weights -> MFMA operand order.  h_W/h_b: HOST arrays of the 10 device
 * weight/bias pointers in module order: pts_linears.{0,2,4,6}, geo_linear.0,
 * rgb_linears.{0,2,4,6}, output_linear.0 (torch layout [out,in]).  packed: device buffer of
 * occnerf_canonical_mlp_packed_floats() floats.  Only mlp_depth = 4, mlp_width = 256
 * (configs/occnerf/zju_mocap/387/occnerf.yaml:16-21) is built. */
int64_t occnerf_canonical_mlp_packed_floats(void);
int occnerf_canonical_mlp_pack(const float *const *h_W, const float *const *h_b, float *packed,
                               void *stream);

/* Geometry + colour trunks on fp32 MFMA.  Replaces occnerf_mlp.py:183-199.
 * mlp_in[N,68] -> raw[N,5] columns 0..3 (rgb logits, sigma); column 4 is left alone.
 * occnerf_canonical_mlp: 16-sample waves (v_mfma_f32_16x16x4_f32), weights staged through LDS -- the
 * default.  occnerf_canonical_mlp_direct: 32-sample waves (32x32x2), weights straight from L2; same
 * packed buffer, same results to fp32 rounding (the dot products associate differently), kept as the
 * cross-check and for A/B timing. */
int occnerf_canonical_mlp(const float *mlp_in, int64_t N, const float *packed, float *raw,
                          void *stream);
int occnerf_canonical_mlp_direct(const float *mlp_in, int64_t N, const float *packed, float *raw,
                                 void *stream);
/* occnerf_canonical_mlp with the row count in DEVICE memory (n_dev, written by occnerf_live_rows on the same
 * stream): the launch covers N_max rows and the workgroups beyond *n_dev leave at once. */
int occnerf_canonical_mlp_counted(const float *mlp_in, int64_t N_max, const int32_t *n_dev,
                                  const float *packed, float *raw, void *stream);

/* The same two trunks on the bf16 matrix pipe with split operands ("bf16x3"): every fp32
 * weight and activation is carried as hi + lo bf16 (16 significand bits) and each product is
 * Wh*xh + Wh*xl + Wl*xh accumulated in fp32 -- 5.3x the fp32-MFMA rate.  Outputs differ from
 * the fp32 kernel by <= ~1e-5 on the raw logits (DESIGN.md section 3.1 has the measured
 * pixel-level effect, two orders inside the 1e-4 gate).  packed = the fp32 blob above (biases,
 * sigma and colour-head rows stay fp32); packed_bf16 = occnerf_canonical_mlp_packed_bf16_bytes()
 * bytes (zero-initialised by the caller: the tail is read-ahead padding) written by
 * occnerf_canonical_mlp_pack_bf16 from the same 10 weight pointers.
 * variant 0: weights staged through LDS by LDS-DMA (the fast one); 1: every wave loads its
 * own operands from L2 (kept for A/B measurements). */
int64_t occnerf_canonical_mlp_packed_bf16_bytes(void);
int occnerf_canonical_mlp_pack_bf16(const float *const *h_W, void *packed_bf16, void *stream);
int occnerf_canonical_mlp_bf16x3(const float *mlp_in, int64_t N, const float *packed,
                                 const void *packed_bf16, float *raw, int32_t variant,
                                 void *stream);
/* The renderer's call (as occnerf_canonical_mlp_rows / _counted for the fp32 kernel): the entry count is read from
 * device memory (*n_dev <= N_max; the launch is sized for N_max), entry n's input row is mlp_in[in_rows[n]]
 * (in_rows nullable: row n), its result goes to raw[n]. */
int occnerf_canonical_mlp_bf16x3_rows(const float *mlp_in, const int32_t *in_rows, int64_t N_max,
                                      const int32_t *n_dev, const float *packed, const void *packed_bf16,
                                      float *raw, int32_t variant, void *stream);

/* Opt-in fp32-GRADE split (cfg.mlp_precision = 'f16x3'): occnerf_mlp.py:183-199 / mlp_offset.py:45-62 on
 * v_mfma_f32_32x32x16_f16 with every operand cut into two fp16 pieces kept in the normal range -- 22 significand bits per
 * operand (fp32: 24), three products, fp32 accumulation (csrc/split.h F16x3: activations travel scaled by 16, the weights'
 * low piece scaled by 2^11 against xh 2^-11; subnormal inputs are preserved by the instruction, measured with
 * tools/mfma_f16_probe.hip).  Domain: hidden activations below 65504 / 16 = 4 094 (larger ones saturate there) -- and leaving
 * it is REPORTED: domain_flag (nullable; a zero-initialised device word the caller owns) has bit 0 set by every wave in which a
 * value reached the clamp, so the caller can re-evaluate with the fp32 kernels (Network.forward does).
 * packed_f16: the same byte count and layout as the bf16 stream (occnerf_canonical_mlp_packed_bf16_bytes /
 * occnerf_nonrigid_packed_bf16_bytes, zero-initialised), written by the _pack_f16 call; packed: the fp32 blob (biases, head
 * rows).  in_rows / rows and n_dev nullable (every row, N_max entries); with a list the count is read from device memory.
 * The non-rigid call may run in place (xyz_out == xyz_in); with rows the offsets go to the listed samples. */
int occnerf_canonical_mlp_pack_f16(const float *const *h_W, void *packed_f16, void *stream);
int occnerf_canonical_mlp_f16x3(const float *mlp_in, const int32_t *in_rows, int64_t N_max, const int32_t *n_dev,
                                const float *packed, const void *packed_f16, float *raw, uint32_t *domain_flag,
                                void *stream);
int occnerf_nonrigid_pack_f16(const float *const *h_W, void *packed_f16, void *stream);
int occnerf_nonrigid_f16x3(const float *xyz_in, int64_t N_max, const int32_t *rows, const int32_t *n_dev,
                           const float *cond, const float *h_hann, const float *W0, const float *b0, float *packed,
                           const void *packed_f16, float *xyz_out, uint32_t *domain_flag, void *stream);

/* Alpha compositing, network.py:320-348.  raw[n,S,5], mask[n*S], z_vals[n,S],
 * rays[n,8] (direction at floats 3..5), h_bgcolor[3] host, 0..255.
 * Outputs rgb[n,3], acc[n], depth[n]; weights[n,S] and term[n] (argmax alpha) optional.
 * out_rows[n] (optional): ray r's rgb / acc / depth / term go to row out_rows[r] (the renderer walks the rays in
 * Morton order and hands the results back in the caller's order without a separate gather). */
int occnerf_composite(const float *raw, const float *mask, const float *z_vals, const float *rays,
                      const float *h_bgcolor, int64_t n, int32_t S, float *rgb, float *acc,
                      float *depth, float *weights, int32_t *term, const int64_t *out_rows, void *stream);

/* ------------------------------------------------------------------------------------
 * 3. Training step (BASELINE configs[4]).  The reference
 *    trains through torch autograd over nn.Linear / F.grid_sample / cumprod (trainer.py:239-249,
 *    occnerf_mlp.py:183-199, network.py:320-402); these are the hand-written forward-with-saved-
 *    activations and backward kernels the autograd Functions of occnerf_amd/train_ops.py call.
 * ---------------------------------------------------------------------------------- */

/* Linear layers on the matrix pipe, element type bf16 (bf16 != 0: v_mfma_f32_32x32x16_bf16, fp32
 * accumulate) or fp32 (v_mfma_f32_32x32x2_f32, exact).  All matrices are row-major with widths padded to
 * multiples of 32 elements (zero padding is exact: padded weights and activations are zeros).
 *
 * occnerf_linear_pack: W[out_dim,in_dim] fp32 (torch layout), b[out_dim] or NULL ->
 *   Wp[n_pad,k_pad] with Wp[n][k] = W[row_map[n]][col_map[k]] (0 where a map entry is -1), Wt[k_pad,n_pad] its
 *   transpose (either may be NULL), bias_p[n_pad] fp32 (may be NULL).  row_map/col_map: int32 device arrays.
 * occnerf_linear_forward: y[m,n] = epi(sum_k x[m,k] W[n,k]), x = [x0 | x1] two column segments (k1 = 0: one),
 *   ld* row pitches in ELEMENTS; epi = (+bias[n]) (ReLU) (zero where mask[m,n] <= 0), each optional;
 *   stored as the element type, or fp32 when out_f32; only columns < n_store are stored;
 *   aux (optional): column aux_col is also written, in fp32, to aux[m * aux_stride].
 *   Forward of a layer: W = Wp, bias, relu.  Input gradient of a layer: x = dZ, W = Wt, mask = the layer's
 *   saved input (its ReLU mask).
 * occnerf_linear_wgrad: part[G,n_pad,k_pad] / dbpart[G,n_pad] = per-workgroup partial sums over row slices of
 *   dZ^T X and of the column sums of dZ, G = occnerf_linear_wgrad_slices(M); occnerf_linear_wgrad_reduce adds
 *   the G slices into dW[out_dim,in_dim] (and db) through the same row/col maps (accumulate != 0: += ). */
int occnerf_linear_pack(const float *W, const float *b, int32_t out_dim, int32_t in_dim, const int32_t *row_map,
                        int32_t n_pad, const int32_t *col_map, int32_t k_pad, int32_t bf16, void *Wp, void *Wt,
                        float *bias_p, void *stream);
int occnerf_linear_forward(const void *x0, int64_t ld0, int32_t k0, const void *x1, int64_t ld1, int32_t k1,
                           const void *W, const float *bias, int32_t relu, const void *mask, int64_t ldm, void *y,
                           int64_t ldy, int32_t out_f32, int32_t n_store, float *aux, int32_t aux_col,
                           int64_t aux_stride, int64_t M, int32_t n_pad, int32_t bf16, void *stream);
int32_t occnerf_linear_wgrad_slices(int64_t M);
int occnerf_linear_wgrad(const void *dz, int64_t lddz, int32_t n_pad, const void *x, int64_t ldx, int32_t k_pad,
                         int64_t M, int32_t bf16, float *part, float *dbpart, void *stream);
int occnerf_linear_wgrad_reduce(const float *part, const float *dbpart, int32_t G, int32_t n_pad, int32_t k_pad,
                                const int32_t *row_map, const int32_t *col_map, float *dW, int32_t in_dim, float *db,
                                int32_t accumulate, void *stream);

/* The training step's forward of BOTH trunks in one launch (csrc/trunks.hip; occnerf_mlp.py:183-199, bf16 arithmetic with fp32
 * accumulation -- BASELINE configs[4]): a sample's activations stay in registers through the ten layers (the renderer's
 * transposed-MFMA scheme) and the tensors the backward reads are written on the way, row-major, exactly as the layer-by-layer
 * forward (occnerf_linear_forward) produced them: X0[M,96] = [agg 35 | var | enc 32 | 0], A1..A4[M,256], GEO[M,96] (geometry
 * features in columns 0..63, sigma in column 64), B1..B4[M,256], all bf16, and raw4[M,4] fp32 = (colour logits, sigma).
 * h_W (host array of device pointers): the nine MFMA layers pts_linears.{0,2,4,6}, geo_linear.0, rgb_linears.{0,2,4,6} in torch
 * layout; packed: occnerf_trunks_packed_bytes() bytes, zero-initialised once by the caller.  packed_f32: the blob of
 * occnerf_canonical_mlp_pack (biases, sigma row, colour rows).  h_A / h_B: host arrays of the four activation buffers. */
int64_t occnerf_trunks_packed_bytes(void);
int occnerf_trunks_pack_bf16(const float *const *h_W, void *packed, void *stream);
int occnerf_trunks_forward_bf16(const float *agg, const float *var, const float *enc, int64_t M, const float *packed_f32,
                                const void *packed_bf16, void *X0, void *const *h_A, void *GEO, void *const *h_B, float *raw4,
                                void *stream);

/* Backward of occnerf_composite (network.py:320-348 under autograd): g_rgb[n,3], g_acc[n], g_depth[n] (each may
 * be NULL = zero) -> d_raw[n*S,5] (column 4 = 0) and d_mask[n*S] (optional).  S <= 256. */
int occnerf_composite_backward(const float *raw, const float *mask, const float *z_vals, const float *rays,
                               const float *h_bgcolor, int64_t n, int32_t S, const float *g_rgb, const float *g_acc,
                               const float *g_depth, float *d_raw, float *d_mask, void *stream);

/* Backward of occnerf_sample_warp's mask output (network.py:351-402 under autograd; x_skel carries no gradient in
 * the reference's graph: it only enters CanonicalMLP through no_grad quantities).  g_mask[n*S] ->
 * d_vol_part[W,nb,G,G,G] and d_rt_part[W,nb,12] (rows: dRs[3,3] then dTs[3]) with
 * W = occnerf_warp_backward_slices(n*S); the caller sums over W.  G must be 32. */
int32_t occnerf_warp_backward_slices(int64_t n_samples);
int occnerf_warp_backward(const float *rays, int64_t n, int32_t S, const float *z_vals, const float *g_mask,
                          const float *Rs, const float *Ts, const float *vol, int32_t nb, int32_t G,
                          const float *h_bbox_min, const float *h_bbox_scale, float *d_vol_part, float *d_rt_part,
                          void *stream);

/* Attention weights of simple_agg (occnerf_mlp.py:110-125): counter[P], knn[N,K] (K <= 40) -> atts[N,K]
 * (softmax) and var[N] (unbiased variance of the normalised counts). */
int occnerf_agg_weights(const float *counter, const int32_t *knn, int64_t N, int32_t K, float *atts, float *var,
                        void *stream);

/* Training step: gradients of the pose refiner's five Linear layers through the chain occnerf_pose_motion_bases evaluates
 * (mlp_delta_body_pose.py:35-41, network_util.py:98-124 Rodrigues, network.py:535-539, network_util.py:166-200 forward
 * kinematics + inverse), given the cotangents dRs[24,3,3], dTs[24,3] of its outputs -- what torch autograd derives in ~460
 * tiny launches per step (trainer.py:239-249).  One workgroup; the forward is recomputed inside.  h_dW[l] / h_db[l]: device
 * buffers shaped like layer l's weight / bias, overwritten.  Only meaningful with refinement on. */
int occnerf_pose_motion_bases_backward(const float *const *h_W, const float *const *h_b, const float *posevec,
                                       const float *dst_Rs, const float *dst_Ts, const float *cnl_gtfms,
                                       const float *dRs, const float *dTs, float *const *h_dW, float *const *h_db,
                                       void *stream);

/* Per-frame preamble.
 * occnerf_pose_motion_bases: pose refiner + motion bases in one launch.  h_W/h_b: HOST arrays of the 5 device weight /
 *   bias pointers of BodyPoseRefiner.block_mlps.{0,2,4,6,8} (69 -> 256 x4 -> 69; mlp_delta_body_pose.py:35-41); refine = 0
 *   skips the refiner (iter_val < pose_decoder.kick_in_iter, network.py:558).  posevec[69], dst_Rs[24,3,3], dst_Ts[24,3],
 *   cnl_gtfms[24,4,4] -> Rs[24,3,3], Ts[24,3] (network_util.py:98-124,166-200; network.py:535-539).
 * occnerf_prior_softmax: vol[C,V] = softmax over C of decoded[C,V] + log(prior[C,V]) (deconv_vol_decoder.py:31-33).
 * occnerf_pack_rays: rays[2,R,3], near[R], far[R] -> rays8[R,8] = (o, d, near, far) of ray order[r] (order NULL: identity). */
int occnerf_pose_motion_bases(const float *const *h_W, const float *const *h_b, const float *posevec, int32_t refine,
                              const float *dst_Rs, const float *dst_Ts, const float *cnl_gtfms, float *Rs, float *Ts,
                              void *stream);
int occnerf_prior_softmax(const float *decoded, const float *prior, int32_t C, int64_t V, float *vol, void *stream);
int occnerf_pack_rays(const float *rays, const float *near, const float *far, const int64_t *order, int64_t R, float *rays8,
                      void *stream);

/* Image assembly after the renderer, run.py:46-63 (unpack_to_image) + image_util.py:19-20 (to_8b_image) in one kernel:
 * out_rgb[H*W*3] = uint8(255 * clip(x, 0, 1)) of the ray's colour where a ray exists, of h_bgcolor01[3] (HOST,
 * cfg.bgcolor / 255 as float32) elsewhere; out_alpha[H*W*3] (optional) the same for alpha, replicated to 3 channels,
 * 0 where no ray.  ray_index[R]: ascending flat pixel index of every ray (nonzero(ray_mask)), int64. */
int occnerf_assemble_image(const float *rgb, const float *alpha, const int64_t *ray_index, int64_t R, int32_t height,
                           int32_t width, const float *h_bgcolor01, uint8_t *out_rgb, uint8_t *out_alpha, void *stream);

/* ConvTranspose3d(kernel 4, stride 2, padding 1) of the motion-weight volume decoder (network_util.py:12-50) as GEMM +
 * gather.  cols[Cout*64, D*H*W] = W.view(Cin, Cout*64)^T x[Cin, D*H*W] (the caller's GEMM) ->
 * out[Cout, 2D, 2H, 2W] = bias[co] + the <= 8 taps that reach each output voxel (occnerf_convt3d_col2im);
 * its adjoint dcols[Cout*64, D*H*W] from gy[Cout, 2D, 2H, 2W] (occnerf_convt3d_im2col), after which
 * dx = W.view(Cin, Cout*64) dcols and dW = x dcols^T are plain GEMMs again.  No atomics, fixed summation order. */
int occnerf_convt3d_col2im(const float *cols, const float *bias, int32_t Cout, int32_t D, int32_t H, int32_t W,
                           float *out, void *stream);
int occnerf_convt3d_im2col(const float *gy, int32_t Cout, int32_t D, int32_t H, int32_t W, float *dcols, void *stream);

/* Optimiser step on the device: the reference's clip_grad_norm_(parameters, max_norm) + torch.optim.Adam.step()
 * (trainer.py:248-249, optimizer.py:12-43) as one multi-tensor pass.  table: n_tensors rows of
 * occnerf_adam_table_row_bytes() = 56 bytes in DEVICE memory, each {float *param; const float *grad; float *exp_avg;
 * float *exp_avg_sq; int64 numel; float lr; float bias_corr1 = 1 - beta1^t; float bias_corr2_sqrt = sqrt(1 - beta2^t);
 * float pad} with t the step count of THAT tensor (torch.optim.Adam keeps one per parameter); chunks[n_chunks,2] int32 =
 * (tensor index, chunk index), a chunk being chunk_elems consecutive elements of its tensor; max_grad_norm <= 0: no clipping.  scratch: n_chunks + 1 floats; scratch[0] receives the squared
 * global gradient norm.  Nothing visits the host. */
int32_t occnerf_adam_table_row_bytes(void);
int occnerf_adam_step(const void *table, int32_t n_tensors, const int32_t *chunks, int32_t n_chunks,
                      int32_t chunk_elems, double beta1, double beta2, double eps, double max_grad_norm, float *scratch,
                      void *stream);

/* LPIPS v0.1, VGG16 trunk (third_parties/lpips/lpips.py:23-124, pretrained_networks.py:96-134): the perceptual term of the
 * reference's training objective (lossweights.lpips, trainer.py:92-106), forward and input gradient in exact fp32.
 * occnerf_lpips_pack: h_conv_w[13] / h_conv_b[13] (HOST arrays of device pointers): the torch weights [Cout,Cin,3,3] and
 *   biases of features.{0,2,5,7,10,12,14,17,19,21,24,26,28}; h_lin[5]: lin0..lin4 weights [1,C,1,1]; shift[3], scale[3]: the
 *   scaling layer -> packed[occnerf_lpips_packed_floats()], the forward and data-gradient operand layouts.  Run once at load.
 * occnerf_lpips_workspace_floats: size of the workspace of one forward/backward pair (-1 for sizes the network refuses).
 * occnerf_lpips_forward: in0, in1 [N,3,H,W] (in_nhwc = 0) or [N,H,W,3] (in_nhwc = 1), H, W >= 16 -> val[N] and, when res is
 *   not NULL, res[5,N] (the per-tap spatial means, retPerLayer).  pred and target run as one batch of 2N images.
 * occnerf_lpips_backward: after the forward on the same workspace; gres[5,N] = d loss / d res (d loss / d val on every tap,
 *   plus the per-tap cotangents) -> d_in0, d_in1 in the inputs' layout, either may be NULL (its half of the batch is skipped).
 * Every pass is bitwise deterministic (split-K partials are summed in a fixed order, no float atomics). */
int64_t occnerf_lpips_packed_floats(void);
int64_t occnerf_lpips_workspace_floats(int32_t N, int32_t H, int32_t W);
int occnerf_lpips_pack(const float *const *h_conv_w, const float *const *h_conv_b, const float *const *h_lin,
                       const float *shift, const float *scale, float *packed, void *stream);
int occnerf_lpips_forward(const float *packed, const float *in0, const float *in1, int32_t N, int32_t H, int32_t W,
                          int32_t in_nhwc, float *work, float *val, float *res, void *stream);
int occnerf_lpips_backward(const float *packed, float *work, int32_t N, int32_t H, int32_t W, int32_t in_nhwc,
                           const float *gres, float *d_in0, float *d_in1, void *stream);

/* Patch images of the training batch, trainer.py:31-41 (_unpack_imgs): img[P,S,S,3] = rgb[row_of_pix[p]] where the pixel has
 * a ray, h_bgcolor01[3] (HOST, bgcolor / 255) elsewhere; row_of_pix[P*S*S] int32, -1 = no ray.  Its adjoint d_rgb[R,3] =
 * d_img[pix_of_row[r]] (each row owns one pixel, so it is a gather). */
int occnerf_patch_assemble(const float *rgb, const int32_t *row_of_pix, int64_t R, int32_t n_patches, int32_t size,
                           const float *h_bgcolor01, float *img, void *stream);
int occnerf_patch_assemble_backward(const float *d_img, const int32_t *pix_of_row, int64_t R, float *d_rgb, void *stream);

/* The training batch of one prepared dataset frame, built on the device: core/data/occnerf/train.py:167-273
 * (get_patch_ray_indices, _get_patch_ray_indices), :322-348 (sample_patch_rays) and the blend of :296-297 + :398.
 * Inputs: image[H,W,3], alpha[H,W,3] uint8 (the frame's PNGs, resident; the occlusion band of :286-287 already applied to
 * alpha), rays8[H*W,8] and box_mask[H*W] as occnerf_gen_rays wrote them.  HOST: h_u[n_patches,2] doubles in [0, 1),
 * subject_ratio = cfg.patch.sample_subject_ratio, h_bgcolor[3] in 0..255.
 * Per patch: u0 < subject_ratio picks the subject class (alpha channel 0 > 0, :470), otherwise box-and-not-subject
 * (:179-182); an EMPTY class falls back to the other one (the reference would raise inside np.random.choice), both empty puts
 * the centre at pixel (0, 0).  The centre is the k-th pixel of the class in row-major order, k = min(floor(u1 * count),
 * count - 1) (np.where's order, :236-242); x_min = clip(cx - size / 2, 0, W - size), y likewise (:245-253).
 * Rows: the patch pixels whose ray hits the box, row-major inside a patch, patches in draw order (:262-273, :214); a pixel
 * inside two overlapping patches gives two rows.  R = the row count <= n_patches * size^2 =: Rmax, which every buffer is sized
 * for.  Outputs: rays[2,Rmax,3], near[Rmax], far[Rmax], target_rgbs[Rmax,3] (rows >= R untouched), target_patches[N,S,S,3]
 * (EVERY pixel blended, :338-343), patch_masks[N,S,S] bytes 0/1, patch_div_indices[N+1], xy_min[N,2] (x, y),
 * pix_of_row[Rmax] = patch * S^2 + y * S + x, row_of_pix[N*S*S] (-1: no ray), n_rows[1] = R.  row_counts[2*H] is scratch.
 * The blend runs in float64 with one rounding per operator, ((a / 255.) * image + (1.0 - a / 255.) * bgcolor) / 255. ->
 * float32, equal to numpy's bit for bit.  Three launches, no atomics, no host wait; size <= 32 is one pass of 1 024 pixels
 * through a 256-thread workgroup per patch (wave64 ballots, one LDS scan across the waves), larger sizes loop. */
int32_t occnerf_patch_batch_max_patches(void);
int occnerf_patch_batch(const uint8_t *image, const uint8_t *alpha, const float *rays8, const uint8_t *box_mask, int32_t H,
                        int32_t W, int32_t n_patches, int32_t size, const double *h_u, double subject_ratio,
                        const float *h_bgcolor, int32_t *row_counts, float *rays, float *near, float *far, float *target_rgbs,
                        float *target_patches, uint8_t *patch_masks, int32_t *patch_div_indices, int32_t *xy_min,
                        int32_t *pix_of_row, int32_t *row_of_pix, int32_t *n_rows, void *stream);

/* A whole frame of a prepared dataset, built on the device: the reference's `ray_shoot_mode 'image'` dict
 * (core/data/occnerf/train.py:353-537 without the patch keys) and the per-pixel maps of eval.py:140-196.
 * Inputs as for occnerf_patch_batch: image[H,W,3], alpha[H,W,3] uint8 (resident, the occlusion band already applied),
 * rays8[H*W,8] and box_mask[H*W] as occnerf_gen_rays wrote them; HOST h_bgcolor[3] in 0..255.  H * W < 2^28.
 * occnerf_whole_frame_count: row_start[H+1] int32 = the number of box pixels in the image rows above each row, row_start[H] = R
 *   (one workgroup per row counts, one workgroup scans the rows in place).  The caller reads R from the device: it sets the
 *   output shapes.
 * occnerf_whole_frame_gather, with that row_start and R: the R rays in row-major pixel order (np.nonzero(ray_mask)'s) --
 *   ray_index[R] int64 (flat pixel index, ascending), rays[2,R,3], near[R], far[R] (copies of rays8), target_rgbs[R,3] (the
 *   float64 blend of occnerf_patch_batch, one rounding per operator, -> float32), ray_alpha[R,3] fp64 = m / 255. -- and, for
 *   EVERY pixel, truth_u8[H,W,3] = uint8(255.f * clip(c, 0, 1)) with c the blended target inside the box and
 *   float32(bgcolor / 255) outside (run.py:46-63 unpack_to_image's truth image), gt_vis[H,W] = float32(m0 / 255.) inside the
 *   box and 0 outside, gt_alpha[H,W] = float32(m0 / 255.), m0 the mask's channel 0.  The body map of the metrics is box_mask.
 *   R = 0 is legal (the ray outputs may then be NULL; the maps are all background).  A row past R is never written.
 * No atomics, no host wait; bit-identical to numpy on the host (PreparedDataset.whole_frame, image.unpack_to_image). */
int occnerf_whole_frame_count(const uint8_t *box_mask, int32_t H, int32_t W, int32_t *row_start, void *stream);
int occnerf_whole_frame_gather(const uint8_t *image, const uint8_t *alpha, const float *rays8, const uint8_t *box_mask,
                               int32_t H, int32_t W, const float *h_bgcolor, const int32_t *row_start, int32_t R,
                               int64_t *ray_index, float *rays, float *near, float *far, float *target_rgbs,
                               double *ray_alpha, uint8_t *truth_u8, float *gt_vis, float *gt_alpha, void *stream);

/* The rays of a camera that has no photograph (freeview / backview / allview / tpose on a prepared dataset): the rays-only
 * form of occnerf_whole_frame_gather.  rays8[H*W,8] and box_mask[H*W] as occnerf_gen_rays wrote them, row_start[H+1] and R
 * from occnerf_whole_frame_count.  One workgroup per image row -> ray_index[R] int64 (flat pixel index, ascending),
 * rays[2,R,3], near[R], far[R] (copies of rays8) in row-major pixel order, np.nonzero(ray_mask)'s.  No image is read and no
 * per-pixel map is written.  R = 0 is legal (the outputs may then be NULL).  A row past R is never written.  H * W < 2^28.
 * No atomics, no host wait. */
int occnerf_view_frame_gather(const float *rays8, const uint8_t *box_mask, int32_t H, int32_t W, const int32_t *row_start,
                              int32_t R, int64_t *ray_index, float *rays, float *near, float *far, void *stream);

/* A photograph (and its mask) undistorted when a prepared dataset is opened: the reference's cv2.undistort(img, K, D) lines
 * (core/data/occnerf/train.py:290-294, allview.py:166-170) as occnerf_amd/undistort.py's undistort_u8 defines them -- OpenCV's
 * undistort -> initUndistortRectifyMap (CV_16SC2 maps, 1/32-pixel fractions) -> remap (INTER_LINEAR, BORDER_CONSTANT 0) with
 * the camera matrix kept, stated as a pure function of the inputs (equality with a particular OpenCV
 * build is not claimed).  image[H,W,3] uint8 on the device; mask[H,W,3] uint8 or NULL (then out_mask is NULL too); HOST
 * h_K[9] (the 3x3 camera matrix as stored, row-major, K[0,1] = 0) and h_dist[8] = (k1, k2, p1, p2, k3, k4, k5, k6), missing
 * coefficients 0, both double.  For every pixel (win_y + r, win_x + c) of the window the source position (u, v) is computed in
 * fp64 with one rounding per operator, quantised to rint(32 u), rint(32 v) (ties to even, saturated to int32; a non-finite
 * position gives 0), and the four taps around it are blended with integer weights that sum to 1024, a tap outside the image
 * reading 0: out = (acc + 512) >> 10 -> out_image[win_h,win_w,3], out_mask[win_h,win_w,3], which must not overlap the inputs.
 * The map is always that of the full image; only the window is written.  One launch, one thread per window pixel, six
 * channels from one map.  H * W < 2^28; the window lies inside the image.  No atomics, no host wait; bit-identical to numpy. */
int occnerf_undistort_u8(const uint8_t *image, const uint8_t *mask, int32_t H, int32_t W, const double *h_K,
                         const double *h_dist, int32_t win_y, int32_t win_x, int32_t win_h, int32_t win_w,
                         uint8_t *out_image, uint8_t *out_mask, void *stream);

/* A prepared frame resized to the training size: the reference's two cv2.resize lines (core/data/occnerf/train.py:306-314) as
 * occnerf_amd/resize.py's resize_blend defines them (equality with a particular OpenCV build is not
 * claimed).  image[H,W,3] uint8 or NULL (then img64 is NULL too: the mask alone), mask[H,W,3] uint8, on the device; HOST
 * h_bgcolor[3] in 0..255 (may be NULL without an image).  The tables are resize.py's resize_tables of both axes and both
 * filters, on the device: x_off_lanczos[w,8] / y_off_lanczos[h,8] int32 clamped source columns / rows with their float32
 * weights x_w_lanczos / y_w_lanczos, and x_off_bilinear[w,2] ... y_w_bilinear[h,2].  h_*_off_*: HOST copies of the four
 * offset tables, which are checked before anything is launched -- an offset outside the image, or y offsets that do not
 * ascend or span more than 24 source rows for one output row, are refused by name.
 * img64[h,w,3] fp64 = the eight-tap Lanczos resize of the float64 blend (m / 255.) * image + (1.0 - m / 255.) * bgcolor (NOT
 * divided by 255, not clipped: it leaves [0, 255] at edges), alpha64[h,w,3] fp64 = the bilinear resize of m / 255.  Both
 * passes are left-to-right sums from 0.0 of double(source) * double(weight), one rounding per operator, the horizontal pass
 * first.  The outputs must not overlap the inputs.  H * W and h * w < 2^28.  One launch: a workgroup computes the horizontal
 * sums of its 32 output columns once into LDS and runs the vertical pass from there.  No atomics, no host wait;
 * bit-identical to numpy. */
int occnerf_resize_frame(const uint8_t *image, const uint8_t *mask, int32_t H, int32_t W, int32_t h, int32_t w,
                         const int32_t *x_off_lanczos, const float *x_w_lanczos, const int32_t *y_off_lanczos,
                         const float *y_w_lanczos, const int32_t *x_off_bilinear, const float *x_w_bilinear,
                         const int32_t *y_off_bilinear, const float *y_w_bilinear, const int32_t *h_x_off_lanczos,
                         const int32_t *h_y_off_lanczos, const int32_t *h_x_off_bilinear, const int32_t *h_y_off_bilinear,
                         const float *h_bgcolor, double *img64, double *alpha64, void *stream);

/* occnerf_patch_batch and occnerf_whole_frame_gather on a frame occnerf_resize_frame has written: img64[H,W,3] and
 * alpha64[H,W,3] fp64 in the place of image and alpha, H x W the training size.  The same kernels with another pixel source:
 * a subject pixel is alpha64[p,0] > 0, the target float32(img64 / 255.) (the background is already blended in; h_bgcolor
 * still colours truth_u8 outside the box), ray_alpha = alpha64, gt_alpha = float32(alpha64[p,0]), gt_vis that value inside
 * the box and 0 outside.  Everything else as documented for the uint8 entries. */
int occnerf_patch_batch_f64(const double *img64, const double *alpha64, const float *rays8, const uint8_t *box_mask,
                            int32_t H, int32_t W, int32_t n_patches, int32_t size, const double *h_u, double subject_ratio,
                            const float *h_bgcolor, int32_t *row_counts, float *rays, float *near, float *far,
                            float *target_rgbs, float *target_patches, uint8_t *patch_masks, int32_t *patch_div_indices,
                            int32_t *xy_min, int32_t *pix_of_row, int32_t *row_of_pix, int32_t *n_rows, void *stream);
int occnerf_whole_frame_gather_f64(const double *img64, const double *alpha64, const float *rays8, const uint8_t *box_mask,
                                   int32_t H, int32_t W, const float *h_bgcolor, const int32_t *row_start, int32_t R,
                                   int64_t *ray_index, float *rays, float *near, float *far, float *target_rgbs,
                                   double *ray_alpha, uint8_t *truth_u8, float *gt_vis, float *gt_alpha, void *stream);

/* Per-frame metrics of the reference's eval.py:100-218 on the 8-bit images of unpack_to_image, N frames of H x W
 * (H, W >= 7) per call.  SSIM is skimage.metrics.structural_similarity(x / 255., y / 255., multichannel=True, full=True)
 * as skimage's source defines it for float64 input: 7x7 uniform filter with scipy's 'reflect' border, sample covariance
 * (49/48), K1 = 0.01, K2 = 0.03, C = (K data_range)^2 (eval.py's float64 images give data_range = 2), evaluated in fp64
 * from exact integer box moments.
 * pred, truth [N,H,W,3] uint8; alpha [N,H,W] float32 (the predicted alpha map, 0 where no ray); body [N,H,W] uint8
 * (ray_mask); gt_vis_alpha [N,H,W] float32 (ray_alpha scattered by ray_mask) or NULL; gt_alpha [N,H,W] float32 (the gt
 * alpha image's channel 0) or NULL.  alpha / body NULL: empty masks.  Masks, compared in float32: vis = gt_vis_alpha > 0.5
 * when given, else alpha > 0.001; IoU = |(alpha > 0.1) & (gt_alpha > 0.5)| / |... or ...| (gt_alpha NULL: nan).
 * record[N, OCCNERF_FRAME_METRICS_RECORD] fp64: psnr_vis, ssim_vis, psnr_body, ssim_body, psnr_full, ssim_full (mssim: the
 * mean with 3 pixels cropped from each edge), iou, then n_vis, n_body, intersection, union (pixels) and the squared-error
 * sums over vis, body, full (8-bit units, all channels).  Empty selections give nan, a zero error inf, as numpy does.
 * ssim_map [N,H,W,3] fp64 (optional): the full S map.  workspace: occnerf_frame_metrics_workspace_bytes(N, H, W) bytes
 * (-1 for sizes the kernel refuses).  Bitwise deterministic (fixed-order sums, no atomics). */
#define OCCNERF_FRAME_METRICS_RECORD 14
int64_t occnerf_frame_metrics_workspace_bytes(int32_t N, int32_t H, int32_t W);
int occnerf_frame_metrics(const uint8_t *pred, const uint8_t *truth, const float *alpha, const uint8_t *body,
                          const float *gt_vis_alpha, const float *gt_alpha, int32_t N, int32_t H, int32_t W,
                          double data_range, double *record, double *ssim_map, void *workspace, void *stream);

/* One frame of the trainer's progress dump (the reference's trainer.py:346-383) written into its tile of the mosaic:
 * the rendered panel -- uint8(255 * clip(x, 0, 1)) of the ray's colour where ray_index[R] (int64, ascending flat pixel index)
 * has the pixel, of h_bgcolor01[3] (HOST, float32(cfg.bgcolor / 255)) elsewhere, exactly occnerf_assemble_image's bytes --
 * to mosaic pixel (tile_y * H + y, tile_x * 2W + x) and truth_u8[H,W,3] to (tile_y * H + y, tile_x * 2W + W + x).
 * mosaic: uint8 [mosaic_rows, mosaic_cols, 3] (sizes in pixels); a tile that does not fit is refused, and no byte outside
 * the tile's H x 2W rectangle is written.  *off_bg (one int32 on the device) = the number of the H*W*3 rendered bytes v with
 * |v - b| > 3 + 1e-5 |b| in fp64, b = h_bgcolor255[3] (HOST, double, cfg.bgcolor as given): 0 exactly when
 * np.allclose(rendered, cfg.bgcolor, atol=3.) holds.  partial: occnerf_progress_tile_blocks(H, W) int32 of workspace (-1 for
 * sizes that are refused: H * W must be below 2^28).  R = 0 is legal (rgb and ray_index may then be NULL): the rendered
 * panel is all background.  Two launches, no atomics, no host wait. */
int32_t occnerf_progress_tile_blocks(int32_t height, int32_t width);
int occnerf_progress_tile(const float *rgb, const int64_t *ray_index, int64_t R, int32_t height, int32_t width,
                          const float *h_bgcolor01, const double *h_bgcolor255, const uint8_t *truth_u8, uint8_t *mosaic,
                          int32_t mosaic_rows, int32_t mosaic_cols, int32_t tile_x, int32_t tile_y, int32_t *partial,
                          int32_t *off_bg, void *stream);

/* The body as a triangle mesh (occnerf_amd/mesh.py, run.py --type mesh).  The reference has no
 * counterpart of these three entries: it exports no geometry.  Marching tetrahedra on the Kuhn split of every cube of
 * field[nz][ny][nx] float32 (x fastest): six tetrahedra per cube around the body diagonal, one per permutation of the axes,
 * so neighbouring cubes agree on every face diagonal and the surface is closed wherever it does not meet the grid's
 * boundary.  A corner is inside iff f > level (strict, in float32: NaN is outside).  A surface vertex lies on one of the 7
 * edge kinds that leave a grid point in a non-negative direction (3 axis edges, 3 face diagonals, the body diagonal) and is
 * named by the int64 key lo_linear * 7 + kind, lo_linear = (z * ny + y) * nx + x, kind = dx + 2 dy + 4 dz - 1.
 * Every axis has at least 2 points and nx * ny * nz < 2^31.  No atomics, no host wait; bit-identical to numpy. */

/* No counterpart in the reference.  row_count[(nz-1)*(ny-1)] int32: the triangles of every row of cubes (z, y): 0, 1 or 2
 * per tetrahedron, at most 12 per cube.  One workgroup per row. */
int occnerf_mesh_count(const float *field, int32_t nx, int32_t ny, int32_t nz, float level, int32_t *row_count,
                       void *stream);
/* No counterpart in the reference.  row_start[(nz-1)*(ny-1)] int64: the exclusive prefix of row_count; T: its total.
 * tri_keys[T,3] int64: the vertex keys of every triangle in the order (z, y, x, tetrahedron 0..5, triangle within the case),
 * wound so that (b - a) x (c - a) points from inside to outside.  A row at or past T is never written.  T = 0 returns 0
 * without a launch (tri_keys may then be NULL). */
int occnerf_mesh_emit(const float *field, int32_t nx, int32_t ny, int32_t nz, float level, const int64_t *row_start,
                      int64_t T, int64_t *tri_keys, void *stream);
/* No counterpart in the reference.  keys[V] int64 (the welded keys) -> pos[V,3] float32: with a the key's lo point and b its
 * other end in grid coordinates, t = (level - fa) / (fb - fa) and p = a + t * (b - a) in fp64, one rounding per operator, a t
 * outside [0, 1] (only non-finite end values give one) replaced by 0.5; pos = float32(h_bbox_min + p * h).  h_bbox_min[3]:
 * HOST, double.  A key that names no edge of the grid gives NaN and reads nothing.  V = 0 returns 0 without a launch. */
int occnerf_mesh_vertices(const int64_t *keys, int64_t V, const float *field, int32_t nx, int32_t ny, int32_t nz,
                          float level, const double *h_bbox_min, double h, float *pos, void *stream);

/* Connected components of a welded triangle mesh (occnerf_amd/mesh.py component_table).  The reference
 * has no counterpart of these two entries.  Two triangles are connected when they share a vertex index; a component is a set
 * of vertices and its label is the smallest vertex index in it; a vertex no face names is a component of its own.  Integer
 * atomics only: every output is a pure function of the inputs, bit-identical to tests/mesh_components_restatement.py.
 * T, V < 2^31. */

/* No counterpart in the reference.  One pass over labels[V] int32, IN/OUT, which the caller starts at labels[v] = v: per
 * triangle of faces[T,3] int32 the smallest of its three labels is written by an atomic minimum into the three vertices and
 * into the vertices their labels name, then every labels[v] is replaced by the top of its chain.  Every store lowers a word
 * and labels[v] <= v holds throughout.  status[2] int32: [0] is set to 1 when the pass lowered a word (the caller zeroes it
 * before the pass and repeats passes until it stays 0: the labels are then final), [1] is set to 1 when a face names a vertex
 * outside [0, V) or labels[] holds a value no pass can have written (such a face or vertex is left alone).  No workgroup
 * waits on another.  V = 0 returns 0 without a launch. */
int occnerf_mesh_label_pass(const int32_t *faces, int64_t T, int64_t V, int32_t *labels, int32_t *status, void *stream);
/* No counterpart in the reference.  The records of the C components, indexed by rank (the components in ascending label
 * order): vrank[V] int32 is the rank of every vertex's component.  With s = llrint(((float64(verts) - h_bbox_min) / h) * 1024)
 * per axis, one rounding per operator, held to [-2^30, 2^30] (NaN: the lower end): counts[C,3] int32 += the component's
 * vertices, triangles (a triangle belongs to the component of its first vertex) and boundary vertices (some s[a] is 0 or
 * (n[a] - 1) * 1024); box[C,6] int32 = min / max with smin[3], smax[3]; vol6[C] int64 += det(s_a, s_b, s_c) over the triangles
 * in two's-complement arithmetic with wrap-around.  The caller zeroes counts and vol6 and fills box with INT32_MAX x 3,
 * INT32_MIN x 3.  h_bbox_min[3]: HOST, double.  Every axis has 2 .. 2^20 points.  A face that names a vertex outside [0, V)
 * and a rank outside [0, C) add nothing.  V = 0 or C = 0 returns 0 without a launch. */
int occnerf_mesh_component_stats(const float *verts, int64_t V, const int32_t *faces, int64_t T, const int32_t *vrank,
                                 int64_t C, const double *h_bbox_min, double h, int32_t nx, int32_t ny, int32_t nz,
                                 int32_t *counts, int32_t *box, int64_t *vol6, void *stream);

/* No counterpart in the reference.  The exported mesh in a frame's pose: x_c[V,3] float32 canonical
 * positions -> p_out[V,3] float32 with F(p) = x_c, F the skeletal warp of occnerf_sample_warp in fp64 on the float32 Rs[nb,3,3],
 * Ts[nb,3], vol[nb,G,G,G] (the background channel dropped) and the HOST h_bbox_min[3] / h_bbox_scale[3].  Per vertex: the bones
 * with a positive trilinear weight at x_c by descending weight (ties: the lower index), at most `candidates` (1..8) of them;
 * per candidate b a damped Newton iteration from R_b^T (x_c - T_b) with the analytic Jacobian, at most max_iter (1..255)
 * steps, each the full step or its first halving (down to 1/32) that lowers max|F(p) - x_c|; converged when that is <= tol
 * and the weight sum >= 1e-4.  flag[V] uint8: 0 converged, 1 not (p_out: the iterate with the smallest residual seen), 2 no
 * bone has a weight at x_c (p_out = x_c); iters[V] uint8: Newton steps spent (saturating); resid[V] float32: max|F(p) - x_c| at
 * the returned p before its rounding to float32.  One rounding per fp64 operator in a fixed order: a pure function of the
 * inputs.  nb <= 32, 2 <= G <= 1024.  V = 0 returns 0 without a launch. */
int occnerf_mesh_pose(const float *x_c, int64_t V, const float *Rs, const float *Ts, const float *vol, int32_t nb, int32_t G,
                      const float *h_bbox_min, const float *h_bbox_scale, int32_t candidates, int32_t max_iter, double tol,
                      float *p_out, uint8_t *flag, uint8_t *iters, float *resid, void *stream);

/* The exported mesh as a rig.  The reference has no counterpart of these two entries.  fp64 on the
 * float32 inputs, one rounding per operator in the order of tests/mesh_rig_restatement.py, no atomics: the same bytes on every run. */

/* No counterpart in the reference.  x_c[V,3] float32 canonical positions -> the K (4 or 8) influences per vertex from the
 * motion-weight volume vol[nb,G,G,G] (the background channel dropped; HOST h_bbox_min[3] / h_bbox_scale[3]): c_b = the
 * trilinear tap of bone b's channel at x_c (that of occnerf_mesh_pose); the bones with c_b > 0 by descending c_b (ties: the
 * lower index), the first n <= K of them; s = their sum in that order, total = sum_b c_b in index order.  joints[V,K] uint8
 * and weights[V,K] float32 = float32(c_k / s) in that order, unused slots joint 0 and weight 0; count[V] uint8 = n; kept[V]
 * float32 = float32(s / total).  n = 0: joint 0 with weight 1, kept 0.  nb <= 32, 2 <= G <= 1024.  V = 0 returns 0 without a
 * launch. */
int occnerf_mesh_skin(const float *x_c, int64_t V, const float *vol, int32_t nb, int32_t G, const float *h_bbox_min,
                      const float *h_bbox_scale, int32_t K, uint8_t *joints, float *weights, uint8_t *count, float *kept,
                      void *stream);
/* No counterpart in the reference.  Forward linear blend skinning of x_c[V,3] with joints[V,K] / weights[V,K] (K 4 or 8) for F
 * frames at once: Rs[F,nb,3,3], Ts[F,nb,3] are the backward bases (observation -> canonical) of the frames;
 * posed[F,V,3] = float32(sum_k w_k R_b^T (x - T_b)) over the slots with w_k != 0, in slot order.  A slot whose joint index is
 * >= nb adds nothing (callers refuse such an index before the call).  With target[F,V,3] float32 and target_flag[F,V] uint8
 * (both or neither; NULL: posed only): M = sum_k w_k R_b^T, M d = target - p (the unrounded p) by Cramer's rule;
 * delta[F,V,3] = float32(d), dflag[F,V] = 0; d = 0 and dflag = 1 where det M is 0 or not finite, target_flag != 0, or not every
 * |d_c| <= max_delta (finite, >= 0).  1 <= F <= 65535, nb <= 32, V < 2^31.  V = 0 returns 0 without a launch. */
int occnerf_mesh_lbs(const float *x_c, int64_t V, const uint8_t *joints, const float *weights, int32_t K, const float *Rs,
                     const float *Ts, int32_t F, int32_t nb, const float *target, const uint8_t *target_flag, double max_delta,
                     float *posed, float *delta, uint8_t *dflag, void *stream);

/* A triangle mesh seen through a pinhole camera (occnerf_amd/mesh_view.py, run.py --type mesh mesh_view.frames; DESIGN.md
 * section 7j).  The reference has no counterpart of these three entries: it draws no geometry.  Bit-identical to
 * tests/mesh_raster_restatement.py; the same bytes on every run.  Limits: 1 <= H, W <= 16384 and H * W <= 2^28; T, V < 2^31. */

/* No counterpart in the reference.  pos[V,3] float32 -> xy[V,2] int32 (the projection in 1/256 pixel, ties to even), z[V]
 * double (the camera-space depth), vflag[V] uint8, with the HOST h_K[9] (row-major 3x3; a skew K[0,1] != 0 is refused) and
 * h_E[16] (row-major 4x4, the camera seen from the space of pos), in fp64, one rounding per operator: c = R p + t;
 * u = fx (c_x / c_z) + cx, v alike.  vflag 1: not c_z >= 1e-3 (NaN included); 2: |256 u| or |256 v| above 2^22, or c_z above
 * 2^20; a flagged vertex has xy = 0 and z = 0.  V = 0 returns 0 without a launch. */
int occnerf_mesh_project(const float *pos, int64_t V, const double *h_K, const double *h_E, int32_t *xy, double *z,
                         uint8_t *vflag, void *stream);
/* No counterpart in the reference.  faces[T,3] int32 over the V projected vertices -> keys[H*W] uint64, IN/OUT: the caller
 * sets every key to all ones (an empty pixel); every covered sample (pixel (i, j) is sampled at (256 j, 256 i); int64 edge
 * functions, top-left rule, two-sided, nothing clipped) lowers its pixel's key to (bits of the float32 perspective-correct
 * depth) << 32 | triangle index by an atomic minimum.  counts[7] int32, zeroed by the caller: triangles dropped for an index
 * outside [0, V) / a vertex with vflag 1 / with vflag 2 / zero fixed-point area / a bounding box off the image, [5] the
 * triangles with more than 64 samples in their clipped box, which a second launch draws with a wave each from wide_list[T]
 * int32 (scratch), [6] is left to occnerf_mesh_resolve.  T = 0 or V = 0 returns 0 without a launch. */
int occnerf_mesh_raster(const int32_t *faces, int64_t T, int64_t V, const int32_t *xy, const double *z, const uint8_t *vflag,
                        int32_t H, int32_t W, uint64_t *keys, int32_t *wide_list, int32_t *counts, void *stream);
/* No counterpart in the reference.  keys[H*W] -> cover[H*W] uint8, tri[H*W] int32 (-1: empty), depth[H*W] float32 (+inf:
 * empty), rgb[H*W,3] uint8: the winner's colors[V,3] uint8 with perspective-correct weights, summed in vertex order and
 * rounded to nearest even; the HOST h_bgcolor[3] uint8 where the pixel is empty.  counts[6] += the covered pixels.  T = 0 or
 * V = 0 returns 0 without a launch (the caller fills the empty image). */
int occnerf_mesh_resolve(const uint64_t *keys, const int32_t *faces, int64_t T, int64_t V, const int32_t *xy, const double *z,
                         const uint8_t *vflag, const uint8_t *colors, const uint8_t *h_bgcolor, int32_t H, int32_t W,
                         uint8_t *cover, int32_t *tri, float *depth, uint8_t *rgb, int32_t *counts, void *stream);

/* The texture of the exported mesh (occnerf_amd/mesh.py bake_texture, run.py --type mesh mesh_texture.enable; DESIGN.md section
 * 7o).  The reference has no counterpart of these three entries.  A per-triangle atlas: with n the cell edge in texels
 * (4 <= n <= 64) and m = n - 3, triangles 2c and 2c + 1 share the n x n cell c at column c % C, row c / C of the atlas; the even
 * one owns the texels (column i, row j) of the cell with i + j <= n - 2, the odd one those with i' + j' <= n - 2, i' = n - 1 - i,
 * j' = n - 1 - j; P = n (n - 1) / 2 texels each, numbered by ascending j', then ascending i' (the even triangle: i' = i, j' = j).
 * Bit-identical to tests/mesh_texture_restatement.py; no atomics, the same bytes on every run. */

/* No counterpart in the reference.  verts[V,3] float32, faces[T,3] int32 -> pts[T,P,3] float32: texel (i', j') of a triangle
 * (v0, v1, v2) is float32(((f64(m - i' - j') v0 + f64(i') v1) + f64(j') v2) / f64(m)) per coordinate, one rounding per fp64
 * operator; the texels (0,0), (m,0), (0,m) reproduce the vertices.  A face with an index outside [0, V): its P rows are NaN
 * and status[0] (int32, zeroed by the caller) becomes 1; no such index is used as an address.  T P < 2^31.  T = 0 returns 0
 * without a launch. */
int occnerf_mesh_texel_points(const float *verts, int64_t V, const int32_t *faces, int64_t T, int32_t n, float *pts,
                              int32_t *status, void *stream);
/* No counterpart in the reference.  rgb[T P,3] float32 (the colours of occnerf_mesh_texel_points' rows) -> the owned texels of
 * atlas[H,W,3] uint8, IN/OUT: uint8(255.0f * min(max(c, 0), 1)) with the product in float32 and truncation, 0 for a NaN; every
 * other byte of the atlas is left as the caller filled it.  W = C n and ceil(ceil(T / 2) / C) n <= H <= 16384 are required.
 * T = 0 returns 0 without a launch. */
int occnerf_mesh_texture_fill(const float *rgb, int64_t T, int32_t n, int32_t C, int32_t H, int32_t W, uint8_t *atlas,
                              void *stream);
/* No counterpart in the reference.  The textured twin of occnerf_mesh_resolve: keys[Himg*Wimg] of occnerf_mesh_raster ->
 * rgb[Himg*Wimg,3] uint8.  A hit pixel: the winner t and its perspective-correct weights as occnerf_mesh_resolve forms them
 * (a vertex with z = 0 is a flagged one), put back into the face's own vertex order; x = min(max(w1 m, 0), m),
 * y = min(max(w2 m, 0), m - x); the taps (floor x + {0,1}, floor y + {0,1}) clamped to [0, n - 1] of t's own frame, weights
 * (1-ax)(1-ay), ax(1-ay), (1-ax)ay, ax ay, each read from atlas[aH,aW,3] through t's cell and, for an odd t, the mirror;
 * s = ((w00 c00 + w10 c10) + w01 c01) + w11 c11 in fp64, rounded to nearest even, clamped to 0..255.  Every other pixel: the
 * HOST h_bgcolor[3] uint8.  The atlas must hold T triangles as occnerf_mesh_texture_fill requires.  T = 0 or V = 0: the
 * background everywhere. */
int occnerf_mesh_resolve_textured(const uint64_t *keys, const int32_t *faces, int64_t T, int64_t V, const int32_t *xy,
                                  const double *z, int32_t Himg, int32_t Wimg, const uint8_t *atlas, int32_t aH, int32_t aW,
                                  int32_t n, int32_t C, const uint8_t *h_bgcolor, uint8_t *rgb, void *stream);

/* The photographs of a prepared dataset on the atlas (occnerf_amd/mesh.py project_photos / export_photo_texture, run.py --type
 * mesh mesh_photo.enable).  The reference has no counterpart of these two entries.  Bit-identical to
 * tests/mesh_photo_restatement.py; integers on the colour path, no atomics (a texel belongs to one thread), the same bytes on
 * every run. */

/* No counterpart in the reference.  One frame onto the accumulators acc[T P,4] int64 (sum of w s per channel, sum of w) and
 * seen[T P] int32, IN/OUT, zeroed by the caller before the first frame.  xy[T P,2] / z[T P] / vflag[T P]: occnerf_mesh_project
 * of occnerf_mesh_texel_points(verts, faces, n); verts[V,3] float32 the posed vertices, pflag[V] uint8 their posing flags;
 * keys[H*W]: occnerf_mesh_raster of the same verts and faces; photo[H*W,3] uint8, inside[H*W] uint8; the HOST h_K[9], h_E[16]
 * as occnerf_mesh_project takes them.  First launch, one thread per triangle -> tri_w[T] int32: with c_k the camera-space
 * vertices, e1 = c1 - c0, e2 = c2 - c0, N = e1 x e2, g = (c0 + c1) + c2, d = N.g, w = min(rint(256 ((d d) / ((N.N)(g.g)))), 256)
 * in fp64, one rounding per operator; 0 when (N.N)(g.g) is 0 or not finite or a vertex carries a posing flag or a flag of
 * occnerf_mesh_project; -1 when d > 0 (the triangle faces away); a face with an index outside [0, V) gets 0 and sets
 * status[0] (int32, zeroed by the caller) to 1, and no such index is used as an address.  Second launch, one thread per texel:
 * seen in this frame when tri_w > 0, vflag == 0, the taps (Y >> 8 + {0,1}, X >> 8 + {0,1}) all lie inside the image, have
 * inside != 0, a key that is not all ones and z <= double(float32 depth of the key) + bias; then with fx = X & 255,
 * fy = Y & 255, s_c = (256-fx)(256-fy) c00 + fx (256-fy) c01 + (256-fx) fy c10 + fx fy c11 (c01 the next column, c10 the next
 * row): acc_c += w s_c, acc_3 += w, seen += 1.  No tap address is formed before the inside-image test.  Refused: a null
 * pointer, n outside 4..64, H or W outside 1..16384, T P >= 2^31, a skew K[0,1] != 0, bias negative or NaN.  T = 0 returns 0
 * without a launch. */
int occnerf_mesh_texture_project(const int32_t *xy, const double *z, const uint8_t *vflag, const float *verts,
                                 const uint8_t *pflag, int64_t V, const int32_t *faces, int64_t T, int32_t n, const double *h_K,
                                 const double *h_E, const uint64_t *keys, const uint8_t *photo, const uint8_t *inside, int32_t H,
                                 int32_t W, double bias, int64_t *acc, int32_t *seen, int32_t *tri_w, int32_t *status,
                                 void *stream);
/* No counterpart in the reference.  One thread per owned texel: seen_img[H,W] uint8 (IN/OUT, zeroed by the caller) receives
 * min(seen, 255) at the texel's place (occnerf_mesh_texture_fill's); atlas[H,W,3] uint8, IN/OUT, the caller's copy of the
 * field's atlas, receives min((acc_c + 32768 acc_3) / (65536 acc_3), 255) in int64 where seen >= min_seen (>= 1) and
 * acc_3 > 0; every other byte stays.  The layout is refused as occnerf_mesh_texture_fill refuses it.  T = 0 returns 0
 * without a launch. */
int occnerf_mesh_texture_blend(const int64_t *acc, const int32_t *seen, int64_t T, int32_t n, int32_t C, int32_t H, int32_t W,
                               int32_t min_seen, uint8_t *atlas, uint8_t *seen_img, void *stream);

/* The tangent-space normal map of the exported mesh (occnerf_amd/mesh.py bake_normal_map, run.py --type mesh mesh_normal.enable;
 * DESIGN.md section 7q).  The reference has no counterpart of these two entries.  Bit-identical to
 * tests/mesh_normal_restatement.py (fp64 on the float32 inputs, one rounding per operator, + - * / sqrt floor rint only); no
 * atomics, the same bytes on every run. */

/* No counterpart in the reference.  One thread per owned texel of the atlas of occnerf_mesh_texture_fill's layout.  verts[V,3],
 * vnormals[V,3] float32 (the mesh's area-weighted vertex normals), faces[T,3] int32, tangents[T,3,4] float32 and creased[T] uint8
 * (mesh.corner_tangents), pts[T P,3] float32 (occnerf_mesh_texel_points), field[nz,ny,nx] float32 with grid point (i,j,k) at
 * h_lo + (i,j,k) h_f (HOST h_lo[3] double), level the iso-value.  Per texel with numerators (b0, b1, b2) = (m - i' - j', i', j'):
 * nh = normalise((b0 N0 + b1 N1) + b2 N2), the face normal and flag 8 when that sum is zero or not finite;
 * f(q) = the trilinear sample at (q - lo) / h_f clamped to [0, n_a - 1], cell min(floor, n_a - 2), x then y then z, each blend
 * a (1 - f) + b f; u_k = f(p + (k delta) nh) - level for k = -S .. S with delta = h_f / 2; a crossing between k and k + 1 where
 * (u > 0) differs and both are finite, s = (k + u_k / (u_k - u_k+1)) delta, the smallest |s| wins, a tie goes to the positive
 * one, none: s = 0 and flag 1; q = p + s nh; g_a = f(q + h_f e_a) - f(q - h_f e_a), N_f = -g / sqrt((gx gx + gy gy) + gz gz),
 * nh and flag 2 when that sum is zero or not finite; Th = normalise of the blended corner tangents, B = nh x Th,
 * (tx, ty, tz) = the solution of tx Th + ty B + tz nh = N_f by cofactors, normalised; |det| < 2^-20, a non-finite solution,
 * tz <= 0 or creased[t] give (0, 0, 1) and flag 4.  atlas[H,W,3] uint8, IN/OUT, receives rint(127.5 (c + 1)) clamped to
 * 0..255 at the texel's place, every other byte stays; offset[T P] float32 = s, flags[T P] uint8, normal[T P,3] float32 = N_f
 * (a NaN is stored as 0x7FC00000).  A face with an index outside [0, V): offset and normal NaN, flags 0, the flat bytes, and
 * status[0] (int32, zeroed by the caller) becomes 1; no such index is used as an address.  Refused: a null pointer, n outside
 * 4..64, T P >= 2^31, an atlas that does not hold T triangles, a grid axis below 2 or 2^31 points, S outside 1..64, h_f not
 * positive and finite.  T = 0 returns 0 without a launch. */
int occnerf_mesh_normal_bake(const float *verts, const float *vnormals, int64_t V, const int32_t *faces, int64_t T,
                             const float *tangents, const uint8_t *creased, const float *pts, int32_t n, int32_t C, int32_t H,
                             int32_t W, const float *field, int32_t nx, int32_t ny, int32_t nz, const double *h_lo, double h_f,
                             float level, int32_t S, uint8_t *atlas, float *offset, uint8_t *flags, float *normal,
                             int32_t *status, void *stream);
/* No counterpart in the reference.  The lit twin of occnerf_mesh_resolve_textured: keys[Himg*Wimg] of occnerf_mesh_raster ->
 * shade_geometry, shade_mapped [Himg*Wimg,3] uint8, both in one launch.  A hit pixel: the winner t and its weights (w0, w1, w2)
 * as occnerf_mesh_resolve_textured forms them; Nh = normalise((w0 N0 + w1 N1) + w2 N2) of vnormals[V,3] float32 (the posed
 * mesh's), Th likewise of tangents[T,3,4] float32, B = Nh x Th; the normal atlas[aH,aW,3] through that entry's sampler with the
 * fp64 blend s kept unrounded, c = s / 127.5 - 1, nm = normalise((cx Th + cy B) + cz Nh), but Nh itself where all four taps are
 * the flat code (128, 128, 255); d = M (column, row, 1) with the HOST h_M[9] double, row major; the grey byte is
 * uint8(255.0f * clamp01(float32(-(n.d) / sqrt(d.d)))) with NaN -> 0, from Nh in shade_geometry and from nm in shade_mapped.
 * Every other pixel: the HOST h_bgcolor[3] uint8.  T = 0 or V = 0: the background everywhere. */
int occnerf_mesh_resolve_lit(const uint64_t *keys, const int32_t *faces, int64_t T, int64_t V, const int32_t *xy,
                             const double *z, int32_t Himg, int32_t Wimg, const float *vnormals, const float *tangents,
                             const uint8_t *atlas, int32_t aH, int32_t aW, int32_t n, int32_t C, const double *h_M,
                             const uint8_t *h_bgcolor, uint8_t *shade_geometry, uint8_t *shade_mapped, void *stream);

/* Collapsed samples, classified once in front of the kNN and feature kernels (no counterpart in the
 * reference).  One lane per entry o of the live list rows[0 .. *n_dev) (capacity N_max): flag[o] = 1 iff xyz[rows[o]] lies
 * inside the radius of center[4] (the |p - c|^2 < r^2 test of the kNN and feature kernels) AND the encoder input x[4] the
 * feature kernel would form for it from the ten neighbours center_idx[0..9] is bitwise center_agg[36..39]; else 0.  For a
 * flagged entry raw_c[o*5+4] = the signed distance the feature kernel would have written.  point_geo: occnerf_point_pack's
 * records (P of them); center / center_idx: occnerf_knn_center's; center_agg: the 72 floats of
 * occnerf_sample_features_centered. */
int occnerf_center_classify(const float *xyz, const int32_t *rows, const int32_t *n_dev, int64_t N_max,
                            const float *point_geo, int32_t P, const float *center, const int32_t *center_idx,
                            const float *center_agg, float bound, float two_bound, uint8_t *flag, float *raw_c,
                            void *stream);
/* The list without its flagged entries, order preserved: keep[o2] = o (the unflagged list positions), rows2[o2] =
 * rows[keep[o2]], *count2 their number, *taken = *n_dev - *count2; in_rows[o] = o2 for a kept entry, centre_row for a flagged
 * one (the input row list of occnerf_canonical_mlp_rows and the split-operand kernels).  keep, rows2, in_rows: N_max entries.
 * temp: occnerf_center_split_temp_bytes(N_max) bytes of device scratch. */
int64_t occnerf_center_split_temp_bytes(int64_t N_max);
int occnerf_center_split(const uint8_t *flag, const int32_t *rows, const int32_t *n_dev, int64_t N_max,
                         int32_t centre_row, int32_t *keep, int32_t *rows2, int32_t *count2, int32_t *in_rows,
                         int32_t *taken, void *temp, int64_t temp_bytes, void *stream);
/* raw_c[keep[o2]*5+4] = raw2[o2*5+4] for o2 < *n2_dev: the kept entries' signed distance back at their list positions. */
int occnerf_center_merge_dist(const float *raw2, const int32_t *keep, const int32_t *n2_dev, int64_t N_max, float *raw_c,
                              void *stream);

/* The geometry the volume renderer sees, per pixel (occnerf_amd/gbuffer.py, run.py show_depth / show_normal / show_shaded /
 * geometry.save).  The reference has no counterpart of these two entries: it drops the compositor's
 * depth.  Everything is float32 with one rounding per operator, division and square root correctly rounded; no atomics, no
 * host wait: bit-identical to tests/gbuffer_restatement.py and the same bytes on every run.  Limits: height * width < 2^31
 * and R <= height * width.
 *
 * ray_index[R] int64 ascending: the flat pixel of every ray (as occnerf_assemble_image takes it); rays[2,R,3]: origins o and
 * unnormalised directions d; depth[R], alpha[R]: the compositor's sum of w z and sum of w.
 * A pixel with ray r is depth-valid iff alpha[r] >= min_alpha, alpha[r] > 0 and both values are finite.  Then
 * t = depth[r] / alpha[r] -- the ray PARAMETER (the reference's depth; the metric distance is t |d|) -- and
 * P_c = o_c + t d_c (product, then sum). */

/* No counterpart in the reference.  One thread per pixel, its ray found by occnerf_assemble_image's binary search ->
 * points[H,W,4] (P, t; zeros where the pixel has no ray or is not depth-valid), valid[H,W] uint8 (bit 0: depth-valid),
 * pix_ray[H,W] int32 (the row r of a depth-valid pixel, else -1).  R = 0: the pointers of the four ray arrays may be NULL. */
int occnerf_gbuffer_points(const int64_t *ray_index, int64_t R, const float *rays, const float *depth, const float *alpha,
                           float min_alpha, int32_t height, int32_t width, float *points, uint8_t *valid, int32_t *pix_ray,
                           void *stream);
/* No counterpart in the reference.  points / pix_ray: occnerf_gbuffer_points' of the same rays.  Per depth-valid pixel (i, j):
 * the horizontal secant a is P(i,j+1) - P (right) or P - P(i,j-1) (left), a candidate existing iff its neighbour is inside
 * the image and depth-valid; of two the one with the smaller |dt| is taken, a tie goes to the right one.  The vertical secant
 * b alike from P(i+1,j) - P (down; it takes the tie) and P - P(i-1,j).  Without a candidate for either the normal is invalid.
 * n = a x b (per component two rounded products and their difference); s = (n_x d_x + n_y d_y) + n_z d_z with the pixel's own
 * d; s > 0: n = -n (towards the camera); l2 = (n_x^2 + n_y^2) + n_z^2, zero or not finite: invalid; else n = n / sqrt(l2) and
 * shade = clamp01(-((n_x d_x + n_y d_y) + n_z d_z) / sqrt((d_x^2 + d_y^2) + d_z^2)), clamp01(x) = min(max(x, 0), 1) and 0
 * for NaN.  The normal is in the space of the rays and is not rotated.
 * -> normal[H,W,3] (zeros where invalid), valid[H,W] uint8 (bit 0 depth-valid, bit 1 normal valid; every byte is written
 * whole and none is read, so occnerf_gbuffer_points' valid may be passed and is finished in place), and the 8-bit panels [H,W,3] through the quantisation of occnerf_assemble_image, each NULL when not wanted:
 * depth_u8 grey clamp01((t_hi - t) / (t_hi - t_lo)) with t_range[2] = (t_lo, t_hi) read from DEVICE memory (NULL only with
 * depth_u8 NULL); normal_u8 0.5 n_c + 0.5; shaded_u8 grey shade.  A pixel that is not depth-valid (depth_u8) or has no
 * valid normal (normal_u8, shaded_u8) gets the HOST h_bgcolor01[3].  R = 0: rays may be NULL. */
int occnerf_gbuffer_normals(const float *points, const int32_t *pix_ray, const float *rays, int64_t R, int32_t height,
                            int32_t width, const float *t_range, const float *h_bgcolor01, float *normal, uint8_t *valid,
                            uint8_t *depth_u8, uint8_t *normal_u8, uint8_t *shaded_u8, void *stream);

/* The driving skeleton of an animate frame as an 8-bit panel (occnerf_amd/skeleton.py, run.py --type animate show_skeleton;
 * DESIGN.md section 7l).  No counterpart in the reference.  Everything is float64 with one rounding per operator and a
 * correctly rounded division; one launch, one thread per pixel, no atomics: bit-identical to tests/skeleton_restatement.py
 * and the same bytes on every run.  All arguments but img and record are HOST pointers, taken by value at the call.
 *
 * h_joints[24,3] float32 in the space of the rays; h_K[3,3] (K[0,1] != 0 is refused), h_E[4,4] float64: camera point
 * c = ((E_r0 x + E_r1 y) + E_r2 z) + E_r3 per row r, u = (K00 c_0) / c_2 + K02, v = (K11 c_1) / c_2 + K12.  A joint with a
 * non-finite c, u or v or with c_2 <= 0 is dropped with the bones that end in it.  Primitive q < 23 is the bone from joint
 * a = q + 1 to its SMPL parent b with radius bone_px and depth key (c_2(a) + c_2(b)) * 0.5; primitive 23 + k is the disc of
 * joint k with radius 1.5 * bone_px and key c_2(k).  Pixel (i, j) is sampled at p = (j, i): with ab = b - a and l2 = ab.ab,
 * s = ((p - a).ab) / l2 clamped to 0..1 (l2 == 0: the disc about a), the sample is covered iff |p - (a + s ab)|^2 <= r^2.
 * Among the covering primitives the smallest key wins, at equal keys the higher index; the pixel gets h_palette[24,3] of the
 * bone's child joint a (of the disc's joint), an uncovered one h_bgcolor[3].
 * -> img[H,W,3] uint8 and record[1 + occnerf_skeleton_panel_blocks(H, W)] int32: record[0] the joints dropped, record[1 + g]
 * the pixels workgroup g covered (the host adds them).  Limits: H, W >= 1, H * W < 2^31, 0 <= bone_px <= 1e6. */
int32_t occnerf_skeleton_panel_blocks(int32_t height, int32_t width);
int occnerf_skeleton_panel(const float *h_joints, const double *h_K, const double *h_E, double bone_px,
                           const uint8_t *h_palette, const uint8_t *h_bgcolor, int32_t height, int32_t width, uint8_t *img,
                           int32_t *record, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OCCNERF_HIP_H */
