"""`Network`: the renderer module, drop-in for core/nets/occnerf/network.py:38-623.

Same constructor (no arguments, reads the global cfg), same `generate_neural_points`,
`deploy_mlps_to_secondary_gpus`, `point_cloud`, `forward(**data, iter_val=...)` keyword
surface and output dict, and the same state_dict key names/shapes,
so a reference checkpoint loads with strict=True.  What differs is how a frame is rendered:

  reference                                         here
  ------------------------------------------------  -----------------------------------------
  ray chunks of 32768 x sample chunks of 300000,    one pass over all samples of the frame
  ~150 torch kernels + pykeops per chunk            (HBM holds them), six HIP kernels
  per-point SDF block recomputed in every chunk     hoisted: once per frame (network.py:263-284)
  fourier embedding of xyz computed, never used     skipped (network.py:287; occnerf_mlp.py:180)
  nn.DataParallel over samples                      one process per GPU, rays sharded
                                                    (occnerf_amd/parallel.py)

Per-frame small stuff (pose decoder, motion bases, motion-weight volume) stays torch
(occnerf_amd/modules.py); everything per sample goes through the C ABI (occnerf_amd/ops.py).
There is no CPU path: forward() raises if the parameters are not on a GPU.
"""
import os
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from . import geometry, ops
from .canonical_mlp import CanonicalMLP
from .config import get_cfg
from .packed import PackedMLPs
from .rayorder import ray_patch_order
from .modules import (BodyPoseRefiner, MotionBasisComputer, MotionWeightVolumeDecoder,
                      NonRigidMotionMLP, hann_window_weights)


class KnnCenter(NamedTuple):
    """A frame's collapse point (Network._knn_center).  center, idx: ops.knn_center's pair, what the kNN kernel's centre cache
    takes.  row: ops.center_row of a sample at the centre (its cached feature row), stamp: what that row was computed from
    (ops.sample_features' freshness contract) -- both None where only the neighbour lists are wanted (the training path)."""
    center: torch.Tensor
    idx: torch.Tensor
    row: Optional[torch.Tensor] = None
    stamp: Optional[tuple] = None


class _Replica(nn.Module):
    """Keeps the `.module.` infix nn.DataParallel puts into the reference's state_dict keys
    (cnl_mlp.module.*, non_rigid_mlp.module.*) without any of its behaviour."""

    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, *a, **k):
        return self.module(*a, **k)


def _load_smpl(cfg):
    """The SMPL body: the licensed model when present, else the synthetic stand-in."""
    choice = cfg.get('smpl_model', 'auto')
    model_dir = './third_parties/smpl/models' if choice in ('auto', 'synthetic') else choice
    pkl = os.path.join(model_dir, 'basicModel_neutral_lbs_10_207_0_v1.0.0.pkl')
    if choice != 'synthetic' and os.path.exists(pkl):
        from third_parties.smpl.smpl_numpy import SMPL   # the user's reference checkout
        return SMPL(sex='neutral', model_dir=model_dir)
    from .synth import SyntheticSMPL
    return SyntheticSMPL()


class Network(nn.Module):
    def __init__(self, avg_betas=None):
        super().__init__()
        cfg = get_cfg()
        self.cfg = cfg
        self.motion_basis_computer = MotionBasisComputer(total_bones=cfg.total_bones)
        self.mweight_vol_decoder = MotionWeightVolumeDecoder(
            embedding_size=cfg.mweight_volume.embedding_size,
            volume_size=cfg.mweight_volume.volume_size, total_bones=cfg.total_bones)
        nr = cfg.non_rigid_motion_mlp
        self.non_rigid_mlp = _Replica(NonRigidMotionMLP(
            pos_embed_size=nr.multires * 6, condition_code_size=nr.condition_code_size,
            mlp_width=nr.mlp_width, mlp_depth=nr.mlp_depth, skips=nr.skips))
        self.pose_decoder = BodyPoseRefiner(
            embedding_size=cfg.pose_decoder.embedding_size, mlp_width=cfg.pose_decoder.mlp_width,
            mlp_depth=cfg.pose_decoder.mlp_depth, total_bones=cfg.total_bones)
        self._ctx = None           # device-side constants of the sample pipeline
        self._ray_orders = {}      # ray_order_key -> (Morton permutation, its inverse)
        self._wconst = None        # decoded volume logits + per-point table (functions of the weights only)
        self._packed = None        # MFMA-ordered MLP weights (eval: cached)

    # ------------------------------------------------------------------ model set-up
    def generate_neural_points(self, avg_betas):
        """network.py:90-146: body points, normals, bound, 3 FPS scales, canonical MLP."""
        cfg = self.cfg
        self.smpl = _load_smpl(cfg)
        betas = np.zeros(10) if avg_betas is None else np.asarray(avg_betas)
        verts, joints = self.smpl(np.zeros(72,), betas)
        try:
            import trimesh
            normals = np.asarray(trimesh.Trimesh(vertices=verts, faces=self.smpl.faces, process=False,
                                                 maintain_order=True).vertex_normals)
        except ImportError:
            normals = geometry.vertex_normals(verts, self.smpl.faces)
        min_xyz = np.min(joints, axis=0) - cfg.bbox_offset
        max_xyz = np.max(joints, axis=0) + cfg.bbox_offset
        self.bound = np.max(np.abs(list(min_xyz) + list(max_xyz)))
        self.detailed_bound = torch.tensor(np.array([list(min_xyz), list(max_xyz)]))

        self.point_base = nn.Parameter(torch.tensor(verts).float(), requires_grad=False)
        self.point_dist = nn.Parameter(torch.zeros(verts.shape[0], 1).float(), requires_grad=True)
        self.point_dist.data.uniform_(-1e-4, 1e-4)
        self.point_counter = nn.Parameter(torch.ones(verts.shape[0]), requires_grad=False)
        self.point_norms = torch.tensor(normals)            # float64, like trimesh's

        self.fps_index, ratio = [], 1.0
        for _ in range(3):                                   # 1/4, 1/16, 1/64 (network.py:113-118)
            ratio /= 4
            self.fps_index.append(torch.from_numpy(geometry.farthest_point_sampling(verts, ratio)))

        self.cnl_mlp = _Replica(CanonicalMLP(
            mlp_depth=cfg.canonical_mlp.mlp_depth, mlp_width=cfg.canonical_mlp.mlp_width,
            input_ch=63, skips=[], bound=self.bound, detailed_bound=self.detailed_bound))
        self._ctx = self._packed = self._wconst = None

    def deploy_mlps_to_secondary_gpus(self):
        return self          # single device per process; rays are sharded across processes

    @property
    def point_cloud(self):
        return self.point_base + self.point_dist

    def _f16x3_flag_word(self):
        """A zero-initialised device word for f16x3 kernels launched outside the render path (the bf16 training step's offsets)."""
        w = self.__dict__.get('_f16x3_word')
        if w is None or w.device != self.point_base.device:
            w = self.__dict__['_f16x3_word'] = torch.zeros(1, device=self.point_base.device, dtype=torch.int32)
        return w

    def _f16x3_enqueue_check(self, flag, what):
        """Copy the flag word to pinned memory behind the work issued so far, clear it, and queue the copy for check_f16x3_domain."""
        self._frames_rendered = getattr(self, '_frames_rendered', 0) + 1
        host = torch.empty(1, dtype=torch.int32, pin_memory=True)
        host.copy_(flag, non_blocking=True)
        flag.zero_()
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(flag.device))
        self.__dict__.setdefault('_f16x3_pending', []).append((done, host, f'{what} {self._frames_rendered}'))

    def check_f16x3_domain(self, wait=True):
        """cfg.f16x3_domain_check = 'deferred': look at the out-of-domain flags of the frames rendered so far (wait=False: only
        those whose copy has completed).  Raises RuntimeError naming the first frame whose activations left the f16x3 domain --
        its pixels were computed with saturated activations and must be rendered again with mlp_precision = 'fp32'."""
        pending = self.__dict__.get('_f16x3_pending')
        while pending:
            done, host, frame_no = pending[0]
            if not wait and not done.query():
                return
            done.synchronize()
            pending.pop(0)
            if int(host[0]) != 0:
                pending.clear()
                raise RuntimeError(f"occnerf_amd: {frame_no} of this Network left the domain of the f16x3 kernels (a hidden activation "
                                   'reached 4 094): its results are not fp32-grade -- use mlp_precision=\'fp32\' / '
                                   "train_nonrigid_f16x3=False (a render with cfg.f16x3_domain_check=True falls back by itself, at the "
                                   'price of one wait per frame)')

    def invalidate_cache(self):
        """Drop the device-side constants and packed weights (load_state_dict and .to() do; in-place weight updates
        are noticed by themselves through the parameters' version counters)."""
        self._ctx = self._packed = self._wconst = None
        self._ray_orders = {}
        # the captured per-step graphs read the dropped constants at baked-in addresses (train_graph.py): drop them too
        self.__dict__.pop('_per_step_graph', None)

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self.invalidate_cache()
        return out

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self.invalidate_cache()
        return out

    # ------------------------------------------------------------------ device constants
    def _context(self):
        """Padded multi-scale point array, index map, float64 normals: constant per model."""
        dev = self.point_base.device
        if self._ctx is not None and self._ctx['device'] == dev:
            return self._ctx
        base = self.point_base.detach()
        P = base.shape[0]
        sets = [torch.arange(P)] + [f.long() for f in self.fps_index]
        rows, imap, begin = [], [], [0]
        for idx in sets:
            pts = base[idx.to(dev)]
            pad = (-pts.shape[0]) % 4                       # +inf rows: never selected
            rows.append(torch.cat([pts, torch.full((pad, 3), float('inf'), device=dev)]))
            imap.append(torch.cat([idx, torch.zeros(pad, dtype=idx.dtype)]))
            begin.append(begin[-1] + pts.shape[0] + pad)
        pts4 = torch.cat(rows)
        pts4 = torch.cat([pts4, torch.zeros(pts4.shape[0], 1, device=dev)], dim=1).contiguous()
        # scale s may reuse the search radius found at scale s+1 when it contains it
        as_sets = [set(s.tolist()) for s in sets]
        seed = [int(l + 1 < len(sets) and as_sets[l + 1] <= as_sets[l]) for l in range(len(sets))]
        normals = self.point_norms.to(dev).double().contiguous()
        cl = geometry.build_knn_clusters(base.cpu().numpy(), [s.numpy() for s in sets])
        clusters = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if k in
                        ('points', 'index_map', 'centers', 'ranges', 'radius', 'group_centers', 'group_ranges', 'group_radius') else v)
                    for k, v in cl.items()}
        self._ctx = {
            'clusters': clusters,
            'device': dev, 'points': pts4, 'index_map': torch.cat(imap).int().to(dev),
            'scale_begin': begin, 'seed': seed, 'normals': normals,
            'unit': ops.unit_normals(normals),
            'bound32': float(np.float32(self.bound)),
            'two_bound32': float(np.float32(2 * np.float64(self.bound))),
        }
        return self._ctx

    def _packed_weights(self):
        """MFMA-ordered MLP weights, repacked whenever a packed parameter changed (optimizer steps update
        the tensors in place: their `_version` counters move, whatever mode the module is in), or cfg.mlp_precision or
        cfg.f16x3_domain_check did: a PackedMLPs (occnerf_amd/packed.py), which also picks the kernels they go to."""
        src = (self.cnl_mlp.module, self.non_rigid_mlp.module, str(self.cfg.get('mlp_precision', 'fp32')),
               self.cfg.get('f16x3_domain_check', True))
        if self._packed is None or self._packed.key != PackedMLPs.cache_key(*src):
            self._packed = PackedMLPs(*src)
        return self._packed

    def _weight_constants(self):
        """Everything of the per-frame preamble that is a function of the weights alone, cached per weight version:
        the decoded motion-weight logits (deconv_vol_decoder.py:25-31: the decoder's input is the constant embedding, only
        `log prior` changes from frame to frame) and the per-point feature table (network.py:263-284 +
        occnerf_mlp.py:171-175, which the reference recomputes in every sample chunk)."""
        dec_mod = self.mweight_vol_decoder
        enc = self.cnl_mlp.module.encoder
        srcs = list(dec_mod.parameters()) + [self.point_dist, self.point_base, enc.embeddings]
        key = tuple((t.data_ptr(), t._version) for t in srcs)
        if self._wconst is not None and self._wconst['key'] == key:
            return self._wconst
        with torch.no_grad():
            dec = dec_mod.decoder.forward_gemm(dec_mod.const_embedding[None])[0].contiguous()
            table = self._point_stage(self._context())
        self._wconst = {'key': key, 'dec': dec, 'table': table}
        return self._wconst

    def _point_pack(self, wc):
        """ops.point_pack of the cached table: per weight version AND per visibility-counter version (the counter moves
        in training steps only, trainer-side validation renders see the new counts)."""
        srcs = [self.point_counter, self.point_base]
        key = (wc['table'].data_ptr(),) + tuple((t.data_ptr(), t._version) for t in srcs)
        if wc.get('pack_key') != key:
            ctx = self._context()
            wc['pack'] = ops.point_pack(self.point_base.detach(), ctx['normals'], ctx['unit'],
                                        self.point_counter.detach(), wc['table'])
            wc['pack_key'] = key
        return wc['pack']

    def _point_stage(self, ctx):
        """network.py:263-284 + occnerf_mlp.py:171-175, once per frame."""
        enc = self.cnl_mlp.module.encoder
        pc = self.point_cloud.detach().float().contiguous()
        base = self.point_base.detach()
        kidx = ops.knn_small(pc, base, 3)
        knn_base, sdf = ops.point_sdf(pc, base, ctx['normals'], ctx['unit'], kidx)
        table = ops.point_table(knn_base, sdf, pc, ctx['bound32'], ctx['two_bound32'],
                                enc.embeddings.detach(), enc.offsets, enc.log2_per_level_scale,
                                enc.base_resolution)
        return table

    # ------------------------------------------------------------------ sample pipeline
    def _sample_features(self, xyz, knn, table, pack=None, **kw):
        """ops.sample_features with the per-model arguments (points, normals, visibility counts, bound, hash grid) filled in."""
        ctx, enc = self._context(), self.cnl_mlp.module.encoder
        return ops.sample_features(
            xyz, knn, self.point_base.detach(), ctx['normals'], ctx['unit'], self.point_counter.detach(), table,
            ctx['bound32'], ctx['two_bound32'], enc.embeddings.detach(), enc.offsets, enc.log2_per_level_scale,
            enc.base_resolution, pack=pack, **kw)

    def _knn_center(self, cond, hann, table=None, pack=None):
        """ops.knn_center's (center, idx) for this frame's collapse point: wherever a sample's motion-weight sum is far below
        the 1e-4 clamp of the reference's warp (network.py:388) its warped position lands within a micrometre of the origin,
        hence -- after the non-rigid offset -- of offset(0): two thirds of a frame's live samples.  The kNN kernel hands those
        queries c's neighbour lists when they lie inside the radius in which the lists provably hold (exact: DESIGN.md 3.2).
        With the frame's table (and point pack) the record also carries c's feature row and what it was computed from."""
        ctx, pk = self._context(), self._packed_weights()
        c = torch.zeros(64, 3, device=self.point_base.device)
        if not self.cfg.ignore_non_rigid_motions:
            # (any point near the cluster serves as c -- the radius is proven for whatever c is searched -- so the first-version
            # kernel's offset(0), equal to the LDS-staged kernel's to fp32 rounding, does; it keeps the per-kernel profiles of the
            # frame's one big nr16 launch clean)
            c = ops.nonrigid(c, cond, hann, pk.nr_w0, pk.nr_b0, pk.nr, direct=True)
        center, idx = ops.knn_center(c[0].contiguous(), ctx['points'], ctx['index_map'], ctx['scale_begin'])
        if table is None:
            return KnnCenter(center, idx)
        # ... and the 36 leading feature columns every sample with c's neighbour lists has (functions of the 40 ids, the
        # visibility counts and the per-point table alone): the feature kernel on samples at c
        row, _, enc_in = self._sample_features(c[:8].contiguous(), idx[None].expand(8, -1, -1).contiguous(), table, pack,
                                               want_enc_in=True)
        return KnnCenter(center, idx, ops.center_row(row[0], enc_in[0]), self._center_stamp(table))

    @staticmethod
    def _put_center_row(mlp_in, at, row):
        """Row `at` of a canonical-MLP input buffer from a KnnCenter.row: ops.center_row's 36 | 4 | 32 layout without the four
        encoder inputs in its middle."""
        mlp_in[at, :36] = row[:36]
        mlp_in[at, 36:] = row[40:72]

    def _center_stamp(self, table):
        return (table.data_ptr(), table._version, self.point_counter._version, self.cnl_mlp.module.encoder.embeddings._version)

    def _render_rays(self, pk, rays8, Rs, Ts, vol, bbox_min, bbox_scale, bgcolor, cond, hann,
                     table, t_rand=None, out=None, out_rows=None, pack=None, boxes=None, center=None):
        """One pass: sample and warp, non-rigid offsets, repeated-sample heads / centre split, kNN, features, canonical MLP,
        results back to their samples, alpha compositing.  pk: the frame's PackedMLPs; center: its KnnCenter or None.
        out: (rgb[R,3], alpha[R], depth[R]) of the whole frame; this pass's rays land in rows out_rows (their index
        in the caller's order) or, without a permutation, in the slice the caller passes."""
        cfg, ctx = self.cfg, self._context()
        S = int(cfg.N_samples)
        t_vals = torch.linspace(0., 1., steps=S, device=rays8.device)
        z, xyz, mask, _ = ops.sample_warp(rays8, S, t_vals, Rs, Ts, vol, bbox_min, bbox_scale,
                                          t_rand=t_rand, boxes=boxes)
        N, dev = xyz.shape[0], xyz.device
        culling = bool(cfg.get('knn_culling', True))
        # Samples whose motion-weight sum is exactly 0 (outside every bone's prior support or outside the
        # canonical volume) cannot contribute: their alpha is multiplied by that sum (network.py:330).  They
        # are dropped here -- a quarter of the samples of the benchmark frame -- and the pixel values are
        # bit-identical to evaluating them (cfg.skip_empty_samples=False; tested).
        # (fp32 and the opt-in split-operand kernels alike: list and count of the live samples stay on the device, no host round
        # trip in the frame.  rows is None: every sample evaluated, cfg.skip_empty_samples off and / or the brute-force
        # neighbour search, cfg.knn_culling off.)
        rows = count = None
        if cfg.get('skip_empty_samples', True) and culling:
            rows, count = ops.live_rows(mask)
            self.last_live_count = count
        if not cfg.ignore_non_rigid_motions:
            pk.offsets(xyz, cond, hann, rows=rows, count=count, out=xyz)
        # Repeated samples (ops.repeat_heads): consecutive live samples with a bitwise identical canonical position
        # share the neighbour search and the features, consecutive feature rows that are bitwise identical share the
        # MLP result.
        # Each distinct input is evaluated once and every sample receives its head's result: bit-identical pixels
        # (cfg.dedup_repeated_samples=False evaluates every live sample; tested).
        dedup = rows is not None and bool(cfg.get('dedup_repeated_samples', True))
        frows, fcount = rows, count             # the list the kNN and feature kernels run on
        if dedup:       # (the positions before the offset differ in their last bits; after it they coincide)
            scan_a, frows, fcount, _ = ops.repeat_heads(xyz, 3, count, rows=rows)
            # (the positions' repeats that are not neighbours in the list are few -- 9.28 M -> 8.39 M on the benchmark
            # frame -- and finding them, 1.7 ms, costs more than the kNN + feature work they save, 0.6 ms)
            if cfg.get('dedup_global_positions', False):
                frows, fcount = ops.unique_heads(xyz, 3, frows, fcount, scan=scan_a, scan_count=count)
        # Collapsed samples (csrc/center.hip; dedup off, the every-live-sample path): a sample inside the centre's radius whose
        # encoder input is bitwise the centre's has the centre's whole feature row -- c's neighbour lists from the kNN kernel,
        # c's 36 aggregate columns and c's 32 encoded ones from the feature kernel.  They are classified once, with a lane each,
        # and leave the list those two kernels run on; the canonical MLP still evaluates every live sample and reads theirs
        # from one centre row behind the compact rows (in_rows).  Same bits (cfg.center_split=False: the path without; tested).
        # A radius of 0 flags nothing.  Counts stay on the device.  cfg.center_split: True / False, default 'auto' = on where
        # the offsets come from the fp32 kernel the centre itself went through (or there are none).  The split-operand non-rigid
        # kernels round differently: the collapsed samples then sit a few 1e-7 m off c, their signed distance differs from c's
        # in its last bits, few are flagged and the stage costs more than it saves (profiles/r09_center_split.md).
        keep = raw_taken = mlp_buf = None
        in_rows, ecount = None, count           # what the canonical MLP evaluates: every listed sample, from its own row
        want = cfg.get('center_split', 'auto')
        if want == 'auto':
            want = pk.nr_split is None or bool(cfg.ignore_non_rigid_motions)
        if rows is not None:
            self.last_center_taken = None
            if not dedup and center is not None and center.row is not None and pack is not None and want:
                M = rows.shape[0]
                raw_taken = torch.empty(M, 5, device=dev)
                flag = ops.center_classify(xyz, rows, count, pack[0], center.center, center.idx, center.row, ctx['bound32'],
                                           ctx['two_bound32'], raw_taken)
                keep, frows, fcount, in_rows, self.last_center_taken = ops.center_split(flag, rows, count, M)
                mlp_buf = torch.empty(M + 1, 68, device=dev)
                self._put_center_row(mlp_buf, M, center.row)
            self.last_head_counts = (fcount, None)
        # (the clustered search: the brute-force one's results with ~5x fewer distance evaluations; its tiles are formed over the
        # listed samples only -- same indices, tested)
        if culling:
            knn = ops.msknn_clustered(xyz, rays8.shape[0], S, ctx['clusters'], ctx['seed'], rows=frows, count=fcount, center=center)
        else:
            knn = ops.msknn(xyz, ctx['points'], ctx['index_map'], ctx['scale_begin'], ctx['seed'])
        # (the feature kernel takes the centre's row on the listed-sample path only, as it always has)
        fcenter = center if rows is not None else None
        if fcenter is not None and fcenter.stamp is not None and fcenter.stamp != self._center_stamp(table):
            raise RuntimeError('stale kNN centre: its cached feature row was computed from another table / counter / embedding '
                               'version than this frame\'s (ops.sample_features freshness contract)')
        mlp_in, raw_c, _ = self._sample_features(
            xyz, knn, table, pack, rows=frows, count=fcount, center=None if fcenter is None else fcenter.center,
            center_agg=None if fcenter is None else fcenter.row, mlp_in_out=mlp_buf)
        del knn
        if keep is not None:        # the kept entries' distance joins the flagged ones': raw_c is complete, in list order
            raw_c = ops.center_merge_dist(raw_c, keep, fcount, raw_taken)
        if dedup:
            scan_b, in_rows, ecount, _ = ops.repeat_heads(mlp_in, 68, fcount)
            if cfg.get('dedup_global', True):       # ... and the repeats that are not neighbours in the list
                in_rows, ecount = ops.unique_heads(mlp_in, 68, in_rows, ecount, scan=scan_b, scan_count=fcount)
            self.last_head_counts = (fcount, ecount)
        # the matrix-pipe kernel (in_rows: the heads' or the centre split's; None without either), its results back to their
        # samples, and the per-ray scan
        raw_e = torch.empty(mlp_in.shape[0], 5, device=dev) if dedup else raw_c
        pk.canonical(mlp_in, raw_e, count=ecount, in_rows=in_rows)
        del mlp_in
        if dedup:
            raw = ops.scatter_raw_heads(raw_e, raw_c, rows, count, scan_a, scan_b, torch.zeros(N, 5, device=dev))
        elif rows is not None:
            raw = ops.scatter_raw(raw_c, rows, count, torch.zeros(N, 5, device=dev))
        else:
            raw = raw_c
        return ops.composite(raw, mask, z, rays8, bgcolor, out=out, out_rows=out_rows)[:3]

    @staticmethod
    def _ray_patch_order(rays_d):
        """Morton walk of the rays (occnerf_amd/rayorder.py): 64 consecutive rays form a compact ~8x8 pixel patch.
        Outputs are returned in the caller's order."""
        return ray_patch_order(rays_d)

    @staticmethod
    def _host3(v):
        """Per-frame float[3] constants (bbox min / scale, background colour) as host float32: the kernels take
        them by value (ops.host_float3: no copy for host arrays, one per tensor object for device tensors)."""
        return ops.host_float3(v)

    @torch.no_grad()
    def live_samples_per_ray(self, rays, dst_Rs, dst_Ts, cnl_gtfms, motion_weights_priors, dst_posevec=None,
                             near=None, far=None, iter_val=1e7, **kwargs):
        """Number of samples with a non-zero motion-weight sum on each of the given rays (int64 [n], on the device, no
        host round trip): the per-frame preamble and the sampler/warp kernel only -- what a frame costs per ray, since
        every later stage runs on the live samples.  occnerf_amd/parallel.py probes a sixteenth of a frame's rays with it
        to deal rays to GPUs by cost."""
        dev = self.point_base.device
        f32 = lambda t: t.detach().float().contiguous().to(dev)          # noqa: E731
        Rs, Ts, vol, boxes = self.render_preamble(
            dict(dst_posevec=dst_posevec, dst_Rs=dst_Rs, dst_Ts=dst_Ts, cnl_gtfms=cnl_gtfms,
                 motion_weights_priors=motion_weights_priors), iter_val, boxes=True)
        rays8 = ops.pack_rays(f32(rays).reshape(2, -1, 3), f32(near).reshape(-1), f32(far).reshape(-1), None)
        S = int(self.cfg.N_samples)
        t_vals = torch.linspace(0., 1., steps=S, device=dev)
        _, _, mask, _ = ops.sample_warp(rays8, S, t_vals, Rs, Ts, vol, self._host3(kwargs['cnl_bbox_min_xyz']),
                                        self._host3(kwargs['cnl_bbox_scale_xyz']), boxes=boxes)
        return (mask.view(-1, S) != 0).sum(dim=1)

    def _require_points(self, name, t):
        """The public point queries take float32 [N,3] on the module's device; name: '<method>: <argument>'.  (Called through
        the class: a host tensor is refused before `self` is looked at -- the wrapper tests pass None for it.)"""
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f'{name} must be a CUDA(HIP) tensor; there is no CPU path')
        if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32:
            raise RuntimeError(f'{name} must be float32 [N,3], got {t.dtype} {tuple(t.shape)}')
        if t.device != self.point_base.device:
            raise RuntimeError(f'{name} is on {t.device}, the module on {self.point_base.device}')

    @torch.no_grad()
    def query_canonical(self, xyz, chunk=1 << 21):
        """raw[N,5] (rgb logits, density logit, signed distance) of the canonical field at xyz [N,3], float32 positions in
        CANONICAL space on the module's device: neighbour search, features and the canonical MLP, the chain a frame's samples
        run through after they have been warped.  No warp and no non-rigid offset is applied: the positions are taken as
        canonical ones, which is what a mesh export wants (occnerf_amd/mesh.py).

        Always the exact fp32 kernels, whatever cfg.mlp_precision says.  The points are evaluated `chunk` at a time (each
        chunk padded to a multiple of 128 by repeating its last point, the padding dropped); every row is a function of its
        own point alone, so the result does not depend on `chunk` bit for bit.  Nothing of the module changes: not its
        train / eval mode, `point_counter`, the renderer's caches or any RNG state."""
        Network._require_points(self, 'query_canonical: xyz', xyz)
        chunk = int(chunk)
        if chunk <= 0:
            raise RuntimeError(f'query_canonical: chunk = {chunk} must be positive')
        S = 128
        chunk = -(-chunk // S) * S
        N, dev = xyz.shape[0], xyz.device
        raw = torch.empty(N, 5, device=dev)
        if N == 0:
            return raw
        ctx = self._context()
        table = self._point_stage(ctx)                 # (this call's own: the renderer's cached constants are left alone)
        pack = ops.point_pack(self.point_base.detach(), ctx['normals'], ctx['unit'], self.point_counter.detach(), table)
        cw, cb = self.cnl_mlp.module.linear_params()
        packed = ops.canonical_mlp_pack(cw, cb)
        xyz = xyz.detach().contiguous()
        for i in range(0, N, chunk):
            n = min(chunk, N - i)
            pad = (-n) % S
            x = xyz[i:i + n]
            if pad:
                x = torch.cat([x, x[-1:].expand(pad, 3)]).contiguous()
            knn = ops.msknn_clustered(x, (n + pad) // S, S, ctx['clusters'], ctx['seed'])
            mlp_in, raw_c, _ = self._sample_features(x, knn, table, pack)
            del knn
            ops.canonical_mlp(mlp_in, packed, raw_c)
            raw[i:i + n] = raw_c[:n]
        return raw

    @torch.no_grad()
    def unoffset_canonical(self, x_c, data, iter_val=1e7, max_iter=10, tol=1e-6):
        """(s [N,3], moving bool [N]): the skeletal-warp output s a frame maps onto the canonical positions x_c [N,3] (float32,
        on the module's device), x_c = s + delta(s; pose) with the frame's non-rigid offset delta -- the fixed point s_0 = x_c,
        s_{k+1} = x_c - delta(s_k), at most `max_iter` rounds or until no coordinate moves by more than `tol` (metres);
        `moving` marks the rows that still did in the last round.  delta comes from the exact fp32 kernel of the renderer
        (ops.nonrigid_rows) with the frame's condition vector and Hann window formed exactly as the render forms them, whatever
        cfg.mlp_precision says.  With cfg.ignore_non_rigid_motions the render applies no offset: s = x_c bit for bit.
        One host wait per round.  Like query_canonical it changes nothing about the module (it packs its own weights)."""
        Network._require_points(self, 'unoffset_canonical: x_c', x_c)
        cfg, dev, N = self.cfg, x_c.device, x_c.shape[0]
        x_c = x_c.detach().contiguous()
        moving = torch.zeros(N, device=dev, dtype=torch.bool)
        if cfg.ignore_non_rigid_motions or N == 0:
            return x_c.clone(), moving
        nr = cfg.non_rigid_motion_mlp
        hann = hann_window_weights(nr.multires, iter_val, nr.kick_in_iter, nr.full_band_iter).tolist()
        posevec = data['dst_posevec'].detach().float().contiguous().to(dev).reshape(-1)
        cond = posevec if iter_val >= nr.kick_in_iter else torch.zeros_like(posevec)
        lin = [m for m in self.non_rigid_mlp.module.block_mlps if isinstance(m, nn.Linear)]
        packed = ops.nonrigid_pack([m.weight.detach() for m in lin], [m.bias.detach() for m in lin])
        w0, b0 = lin[0].weight.detach(), lin[0].bias.detach()
        rows = torch.arange(N, device=dev, dtype=torch.int32)
        count = torch.full((1,), N, device=dev, dtype=torch.int32)
        s = x_c.clone()
        for _ in range(int(max_iter)):
            y = ops.nonrigid_rows(s.clone(), rows, count, cond, hann, w0, b0, packed)      # s + delta(s)
            nxt = x_c - (y - s)
            moving = (nxt - s).abs().amax(dim=1) > float(tol)
            s = nxt
            if not bool(moving.any()):
                break
        return s, moving

    @torch.no_grad()
    def render_preamble(self, data, iter_val=1e7, boxes=False):
        """(Rs[24,3,3], Ts[24,3], vol[25,G,G,G]) of a frame (the fused kernels of csrc/preamble.hip): what the render branch of
        `forward` and `live_samples_per_ray` run on -- and parity tools that feed a checker the same per-frame outputs.
        boxes=True: a fourth entry, what ops.sample_warp takes as `boxes`."""
        f32 = lambda t: t.detach().float().contiguous().to(self.point_base.device)          # noqa: E731
        wc = self._weight_constants()
        refine = iter_val >= self.cfg.pose_decoder.get('kick_in_iter', 0)
        Rs, Ts = ops.pose_motion_bases(self.pose_decoder, f32(data['dst_posevec']).reshape(-1), refine, f32(data['dst_Rs']),
                                       f32(data['dst_Ts']), f32(data['cnl_gtfms']))
        vol = ops.prior_softmax(wc['dec'], f32(data['motion_weights_priors']))
        if not boxes:
            return Rs, Ts, vol
        # support box of every bone's weight channel (one tiny launch): the warp kernel skips the bones that cannot
        # reach a wave's samples -- same bits (cfg.warp_bone_culling=False: every bone for every sample)
        return Rs, Ts, vol, (ops.bone_boxes(vol, Rs.shape[0]) if self.cfg.get('warp_bone_culling', True) else None)

    def forward(self, rays, dst_Rs, dst_Ts, cnl_gtfms, motion_weights_priors, dst_posevec=None,
                near=None, far=None, iter_val=1e7, **kwargs):
        cfg = self.cfg
        dev = self.point_base.device
        if dev.type != 'cuda':
            raise RuntimeError('occnerf_amd.Network renders on a GPU only; move the module with '
                               '.cuda() first (the reference has no CPU path either)')
        want_grad = torch.is_grad_enabled()
        # fused HIP render when no graph is wanted and the module is in eval mode; the staged differentiable
        # path otherwise (training mode under no_grad still produces comp_loss and the counter update, as the
        # reference's `if self.training` branch does, network.py:486)
        fused = not want_grad and not self.training
        R = int(near.numel())
        shape = list(rays[1].shape[:-1])
        if R == 0:                                   # a rank's empty shard / a frame that misses the bbox
            z = torch.zeros(0, device=dev)
            return {'rgb': z.reshape(shape + [3]), 'alpha': z.reshape(shape), 'depth': z.reshape(shape),
                    'comp_loss': torch.zeros(0 if self.training else 1, device=dev)}

        nr = cfg.non_rigid_motion_mlp
        hann = hann_window_weights(nr.multires, iter_val, nr.kick_in_iter, nr.full_band_iter)       # host
        refine = iter_val >= cfg.pose_decoder.get('kick_in_iter', 0)
        bbox_min = self._host3(kwargs['cnl_bbox_min_xyz'])
        bbox_scale = self._host3(kwargs['cnl_bbox_scale_xyz'])
        bgcolor = self._host3(kwargs['bgcolor'])
        S = int(cfg.N_samples)
        rays_o, rays_d = rays

        def morton_order(dirs):
            """Morton order of the rays (kNN tiles, gather locality).  It depends on the camera only: a caller that
            renders many frames from one camera (movement sequences, the benchmark) names it with
            ray_order_key=<hashable> and the permutation (an argsort of R keys) is computed once."""
            if not cfg.get('ray_patch_order', True):
                return None
            key = kwargs.get('ray_order_key')
            hit = self._ray_orders.get(key) if key is not None else None
            if hit is not None and hit.numel() == R and hit.device == dirs.device:
                return hit
            order = self._ray_patch_order(dirs)
            if key is not None:
                if len(self._ray_orders) >= 8:
                    self._ray_orders.clear()
                self._ray_orders[key] = order
            return order

        if fused:
            # ---- render: 3 launches of per-frame preamble (csrc/preamble.hip), then the sample pipeline ----
            self.check_f16x3_domain(wait=False)      # (cfg.f16x3_domain_check = 'deferred': earlier frames whose flag has arrived)
            with torch.no_grad():
                wc = self._weight_constants()
                pack = self._point_pack(wc)
                f32 = lambda t: t.detach().float().contiguous()          # noqa: E731
                cond = f32(dst_posevec).reshape(-1) if iter_val >= nr.kick_in_iter else \
                    torch.zeros(dst_posevec.numel(), device=dev)
                pk = self._packed_weights()      # the frame's MLP weights and kernels: taken once, handed down
                # The collapse point's chain (its non-rigid offset, its neighbour lists and radius, its feature row: three
                # single-workgroup kernels) runs on the caller's stream like everything else.  (Round 5 carried an opt-in
                # side-stream placement and a two-stream chunk pipeline; both measured neutral to negative and were removed in
                # round 6 -- the renderer uses ONE stream, HISTORY.md 3.7.)
                center = None
                if cfg.get('knn_center_cache', True) and cfg.get('knn_culling', True):
                    center = self._knn_center(cond, hann.tolist(), wc['table'], pack)
                Rs, Ts, vol, boxes = self.render_preamble(
                    dict(dst_posevec=dst_posevec, dst_Rs=dst_Rs, dst_Ts=dst_Ts, cnl_gtfms=cnl_gtfms,
                         motion_weights_priors=motion_weights_priors), iter_val, boxes=True)
                rays_f = f32(torch.stack([rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)]) if not torch.is_tensor(rays) else
                             rays.reshape(2, -1, 3))
                order = morton_order(rays_f[1])
                rays8 = ops.pack_rays(rays_f, f32(near).reshape(-1), f32(far).reshape(-1), order)
                out = (torch.empty(R, 3, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev))
                # all rays of the frame in as few passes as memory allows
                cap = int(cfg.get('max_samples_per_pass', 1 << 28))
                if R * S > (1 << 26):      # (a frame of > 30 GB: ~470 B per resident sample, at most half of what is free)
                    # free = what the driver reports + the allocator's cached, reusable blocks (after the first large frame
                    # the cache holds the frame's buffers: counting them as used would split later frames further)
                    free = (torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev)
                            - torch.cuda.memory_allocated(dev))
                    cap = min(cap, max(1 << 22, int(free // 2 // 470)))
                rays_per_pass = max(1, cap // S)

                def passes(pk):
                    for i in range(0, R, rays_per_pass):
                        n = min(rays_per_pass, R - i)
                        dst = {'out': out, 'out_rows': order[i:i + n]} if order is not None else \
                            {'out': tuple(t[i:i + n] for t in out)}
                        self._render_rays(pk, rays8[i:i + n], Rs, Ts, vol, bbox_min, bbox_scale, bgcolor, cond, hann.tolist(),
                                          wc['table'], pack=pack, boxes=boxes, center=center, **dst)
                passes(pk)
                # f16x3 is exact-grade only inside its domain (hidden activations below 4 094: csrc/split.h); its kernels report
                # leaving it -- never silently wrong pixels.  cfg.f16x3_domain_check: True / 'sync' (default) reads the flag after
                # the frame (the read waits for the frame) and renders the frame AGAIN with the fp32 kernels when it is set (on the
                # same packed weights' fp32 view: nothing is packed again, cfg is not touched);
                # 'deferred' copies the flag to pinned memory behind the frame and looks at it when a later frame starts (or in
                # check_f16x3_domain()): no wait in a pipelined loop, and a violation RAISES there, naming the frame, because
                # that frame's pixels have already been handed out; False skips the check and the guarantee.
                mode = cfg.get('f16x3_domain_check', True)
                flag = pk.domain_flag if (R > 0 and mode) else None
                if flag is not None and mode == 'deferred':
                    self._f16x3_enqueue_check(flag, 'frame')
                elif flag is not None and int(flag.item()) != 0:
                    flag.zero_()
                    self.f16x3_fallback_frames = getattr(self, 'f16x3_fallback_frames', 0) + 1
                    if self.f16x3_fallback_frames == 1:
                        import warnings
                        warnings.warn("occnerf_amd: a hidden activation left the domain of cfg.mlp_precision='f16x3' (>= 4 094); "
                                      'this frame -- and every later one that does -- is rendered again with the fp32 kernels')
                    passes(pk.exact())
                rgb, acc, depth = out
                comp_loss = torch.zeros(1, device=dev)
        else:
            # ---- differentiable path: per-frame modules in torch (gradients to the pose refiner and the volume
            # decoder), then HIP forward + HIP backward per stage (train_path.py) ----
            from . import train_path
            dst_Rs, dst_Ts = dst_Rs[None], dst_Ts[None]
            dst_posevec, cnl_gtfms = dst_posevec[None], cnl_gtfms[None]
            motion_weights_priors = motion_weights_priors[None]
            self.check_f16x3_domain(wait=False)      # (the bf16 step's f16x3 offsets: flags of earlier steps that have arrived)
            with torch.set_grad_enabled(want_grad):
                # the per-frame modules always run in fp32 (bone transforms in bf16 would move every sample); a caller's
                # torch.autocast(bfloat16) selects the arithmetic of the MLP trunks only (train_path._use_bf16)
                with torch.autocast('cuda', enabled=False):
                    dst_Rs, dst_Ts, cnl_gtfms = dst_Rs.float(), dst_Ts.float(), cnl_gtfms.float()
                    dst_posevec = dst_posevec.float()
                    cond = dst_posevec if iter_val >= nr.kick_in_iter else torch.zeros_like(dst_posevec)
                    static = None
                    if want_grad and cfg.get('train_graph', True):
                        # pose refiner, Rodrigues, motion bases, volume decoder and the per-point SDF block
                        # -- ~250 tiny launches forward, ~450 backward -- replayed as two hipGraphs (train_graph.py)
                        from . import train_graph
                        static = train_graph.get(self)(refine, dst_posevec, dst_Rs, dst_Ts, cnl_gtfms, motion_weights_priors)
                    if static is not None:
                        Rs, Ts, vol, knn_base, point_sdf = static
                    else:
                        Rs, Ts = train_path.motion_bases(self, refine, dst_posevec, dst_Rs, dst_Ts, cnl_gtfms)
                        vol = self.mweight_vol_decoder(motion_weights_priors=motion_weights_priors.float())[0]
                        knn_base, point_sdf = train_path.point_sdf_block(self)      # once per step (the reference: every chunk)
                rays8 = torch.cat([rays_o.reshape(-1, 3).float(), rays_d.reshape(-1, 3).float(),
                                   near.reshape(-1, 1).float(), far.reshape(-1, 1).float()], -1)
                order = morton_order(rays8[:, 3:6])
                rays8 = (rays8[order] if order is not None else rays8).contiguous()
                t_rand = kwargs.get('t_rand')            # optional injected jitter [R,S] (tests)
                if t_rand is not None and order is not None:
                    t_rand = t_rand[order]
                outs = []
                for i in range(0, rays8.shape[0], int(cfg.chunk)):
                    outs.append(train_path.render_rays_autograd(
                        self, rays8[i:i + cfg.chunk], Rs, Ts, vol, bbox_min, bbox_scale, bgcolor, cond.float(),
                        hann.tolist(), None if t_rand is None else t_rand[i:i + cfg.chunk], point_block=(knn_base, point_sdf)))
                rgb, acc, depth, comp_loss = (torch.cat(t, 0) if len(outs) > 1 else outs[0][j]
                                              for j, t in enumerate(zip(*outs)))
                if order is not None:            # back to the caller's ray order
                    inv = torch.empty_like(order)
                    inv[order] = torch.arange(order.numel(), device=order.device)
                    rgb, acc, depth = rgb[inv], acc[inv], depth[inv]
                    if comp_loss.shape[0] == order.numel():
                        comp_loss = comp_loss[inv]
        return {'rgb': rgb.reshape(shape + [3]), 'alpha': acc.reshape(shape),
                'depth': depth.reshape(shape),
                'comp_loss': comp_loss.reshape(-1)}
