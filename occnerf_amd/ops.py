"""Torch-facing wrappers of the C ABI (include/occnerf_hip.h).

Each function validates its tensors (GPU, contiguous, dtype -- the reference's
CHECK_CUDA / CHECK_CONTIGUOUS / CHECK_IS_* of gridencoder.cu:15-18, raised as
RuntimeError), allocates outputs with torch, and launches on torch's current stream of
the tensors' device.  PyTorch is plumbing here: memory, streams, device guard.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

_f32p = C.POINTER(C.c_float)


def _chk(t, dtype, name):
    if not torch.is_tensor(t):
        raise RuntimeError(f'{name} must be a tensor')
    if not t.is_cuda:
        raise RuntimeError(f'{name} must be a CUDA(HIP) tensor; there is no CPU path')
    if not t.is_contiguous():
        raise RuntimeError(f'{name} must be a contiguous tensor')
    if t.dtype != dtype:
        raise RuntimeError(f'{name} must be {dtype}, got {t.dtype}')
    return t.data_ptr()


def _guard_dev(dev):
    if torch.device(dev).type != 'cuda':
        raise RuntimeError(f'tensors are on {dev}: this path runs on a GPU only, there is no CPU path')
    return torch.cuda.device(dev)


def _guard(t):
    if not torch.is_tensor(t):
        raise RuntimeError('expected a tensor')
    return _guard_dev(t.device)


def _opt(t, dtype, name):
    return None if t is None else _chk(t, dtype, name)


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _host_f32(vals, n):
    a = np.ascontiguousarray(np.asarray(vals, dtype=np.float32).ravel())
    assert a.size == n, (a.size, n)
    return a, a.ctypes.data_as(C.c_void_p)


def _host_i32(vals):
    a = np.ascontiguousarray(np.asarray(vals, dtype=np.int32).ravel())
    return a, a.ctypes.data_as(C.c_void_p)


class _HostCopies:
    """Host copies of small constant device tensors (level offsets, per-frame float[3] constants), fetched with
    one blocking copy the first time a tensor OBJECT is seen.  Keyed by object identity (checked through a weak
    reference) and version counter -- never by device address, which the caching allocator recycles."""

    def __init__(self, limit=256):
        self._items, self._limit = {}, limit

    def get(self, t, convert):
        import weakref
        hit = self._items.get(id(t))
        if hit is not None and hit[0]() is t and hit[1] == t._version:
            return hit[2]
        if len(self._items) > self._limit:
            self._items = {k: v for k, v in self._items.items() if v[0]() is not None}
            if len(self._items) > self._limit:
                self._items.clear()
        val = convert(t)
        self._items[id(t)] = (weakref.ref(t), t._version, val)
        return val


_host_copies = _HostCopies()


def _host_offsets(offsets):
    """Host copy of a (constant) level-offset tensor, fetched once per tensor object."""
    def convert(t):
        a = np.ascontiguousarray(t.detach().cpu().numpy().astype(np.int32))
        return a, a.ctypes.data_as(C.c_void_p)
    return _host_copies.get(offsets, convert)[1]


def host_float3(v):
    """float[3] per-frame constant (bbox min / scale, background colour) as host float32: free for host arrays,
    one blocking copy per tensor object for device tensors."""
    if torch.is_tensor(v):
        return _host_copies.get(v, lambda t: np.asarray(t.detach().cpu().numpy(), dtype=np.float32).reshape(3).copy())
    return np.asarray(v, dtype=np.float32).reshape(3)


def _ptr_table(tensors, name):
    ptrs = [_chk(t, torch.float32, f'{name}[{i}]') for i, t in enumerate(tensors)]
    arr = (C.c_void_p * len(ptrs))(*ptrs)
    return arr


# ------------------------------------------------------------------ grid encoder (section 1)
def _encoder_dtype(t, what):
    """gridencoder.cu:467,500 dispatch on the tensor dtype over float / double / half (grid.py:42-45 feeds half embeddings
    under autocast): all three cases of AT_DISPATCH_FLOATING_TYPES_AND_HALF are built (csrc/grid_encode.hip)."""
    if t.dtype not in (torch.float32, torch.float16, torch.float64):
        raise RuntimeError(f'{what}: tensors are {t.dtype}; gridencoder.cu:467 dispatches float32, float64 and float16')
    return t.dtype


# entry-point suffix per dtype; fp32 takes the `_h` entries, which also get the host copy of the offsets
_ENCODER_ENTRY = {torch.float32: '_h', torch.float16: '_f16', torch.float64: '_f64'}


def grid_grad_runs(grad_rows, inputs, B, D, L, Cc):
    """grad_rows[B, L*C] fp32 -> [L,B,C] with the rows of runs of bitwise identical inputs summed into the run's first sample."""
    out = torch.empty(L, B, Cc, device=grad_rows.device, dtype=torch.float32)
    with _guard(grad_rows):
        rc = _lib.lib().occnerf_grid_grad_runs(_chk(grad_rows, torch.float32, 'grad_rows'), _chk(inputs, torch.float32, 'inputs'),
                                               int(B), int(D), int(L), int(Cc), out.data_ptr(), _stream(grad_rows))
    _lib.check(rc, 'grid_grad_runs')
    return out


def grid_encode_forward(inputs, embeddings, offsets, outputs, B, D, Cc, L, S, H, dy_dx=None,
                        gridtype=0, align_corners=False, interp=0):
    """Same positional signature as the reference's `_gridencoder.grid_encode_forward`
    (bindings.cpp:6); writes `outputs[L,B,C]` (and `dy_dx`) in place.  Dispatches on embeddings.dtype like the reference."""
    dt = _encoder_dtype(embeddings, 'grid_encode_forward')
    fp32 = dt == torch.float32
    with _guard(inputs):
        args = [_chk(inputs, torch.float32, 'inputs'), _chk(embeddings, dt, 'embeddings'), _chk(offsets, torch.int32, 'offsets')]
        if fp32:
            args.append(_host_offsets(offsets))
        rc = getattr(_lib.lib(), 'occnerf_grid_encode_forward' + _ENCODER_ENTRY[dt])(
            *args, _chk(outputs, dt, 'outputs'), int(B), int(D), int(Cc), int(L), float(S), int(H), _opt(dy_dx, dt, 'dy_dx'),
            int(gridtype), int(bool(align_corners)), int(interp), _stream(inputs))
    _lib.check(rc, 'grid_encode_forward')


def grid_encode_backward(grad, inputs, embeddings, offsets, grad_embeddings, B, D, Cc, L, S, H,
                         dy_dx=None, grad_inputs=None, gridtype=0, align_corners=False, interp=0):
    """`_gridencoder.grid_encode_backward` (bindings.cpp:7); dispatches on grad.dtype like the reference (:500)."""
    dt = _encoder_dtype(grad, 'grid_encode_backward')
    fp32 = dt == torch.float32
    # room for the tile-set pre-pass of the tiled backward (large D = 4, C = 2 batches only)
    scratch = torch.empty(int(L) * int(B), device=inputs.device, dtype=torch.int64) if (fp32 and int(D) == 4 and int(Cc) == 2
                                                                                      and int(B) >= 32768) else None
    with _guard(inputs):
        args = [_chk(grad, dt, 'grad'), _chk(inputs, torch.float32, 'inputs'), _chk(embeddings, dt, 'embeddings'),
                _chk(offsets, torch.int32, 'offsets')]
        if fp32:
            args.append(_host_offsets(offsets))
        args += [_chk(grad_embeddings, dt, 'grad_embeddings'), int(B), int(D), int(Cc), int(L), float(S), int(H),
                 _opt(dy_dx, dt, 'dy_dx'), _opt(grad_inputs, dt, 'grad_inputs'), int(gridtype), int(bool(align_corners)),
                 int(interp)]
        if fp32:
            args += [None if scratch is None else scratch.data_ptr(), 0 if scratch is None else scratch.numel() * 8]
        rc = getattr(_lib.lib(), 'occnerf_grid_encode_backward' + _ENCODER_ENTRY[dt])(*args, _stream(inputs))
    _lib.check(rc, 'grid_encode_backward')


def grad_total_variation(inputs, embeddings, grad, offsets, weight, B, D, Cc, L, S, H, gridtype=0,
                         align_corners=False):
    """`_gridencoder.grad_total_variation` (bindings.cpp:8): exported, not implemented."""
    rc = _lib.lib().occnerf_grad_total_variation(None, None, None, None, float(weight), int(B), int(D),
                                                 int(Cc), int(L), float(S), int(H), int(gridtype),
                                                 int(bool(align_corners)), None)
    _lib.check(rc, 'grad_total_variation')


# ------------------------------------------------------------------ per-frame ray generation
def _host_f64(vals, n):
    a = np.ascontiguousarray(np.asarray(vals, dtype=np.float64).ravel())
    assert a.size == n, (a.size, n)
    return a, a.ctypes.data_as(C.c_void_p)


def gen_rays(K, E, H, W, bbox_min, bbox_max, device, out=None):
    """All H*W pixel rays of a camera on the device -> rays8[H*W,8] (o, d, near, far), mask[H*W] uint8.
    out=(rays8, mask): write into these buffers instead of new ones (the patch batch loader's resident pair)."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError(f'gen_rays: needs a GPU device, got {dev}')
    f32 = int(np.asarray(K).dtype == np.float32 and np.asarray(E).dtype == np.float32)   # numpy's result dtype
    E = np.asarray(E, dtype=np.float64)
    k0, pk = _host_f64(np.linalg.inv(np.asarray(K)).astype(np.float64), 9)      # inverse in K's own dtype
    r0, pr = _host_f64(E[:3, :3], 9)
    t0, pt = _host_f64(E[:3, 3], 3)
    l0, pl = _host_f64(bbox_min, 3)
    h0, ph = _host_f64(bbox_max, 3)
    if out is None:
        rays8 = torch.empty(H * W, 8, device=dev, dtype=torch.float32)
        mask = torch.empty(H * W, device=dev, dtype=torch.uint8)
    else:
        rays8, mask = out
        _chk(rays8, torch.float32, 'rays8'), _chk(mask, torch.uint8, 'mask')
        if rays8.numel() != H * W * 8 or mask.numel() != H * W or rays8.device != mask.device:
            raise RuntimeError(f'gen_rays: out must be rays8[{H * W},8] and mask[{H * W}] on one device')
    with _guard_dev(rays8.device):
        rc = _lib.lib().occnerf_gen_rays(pk, pr, pt, f32, int(H), int(W), pl, ph, rays8.data_ptr(),
                                         mask.data_ptr(), _stream(rays8))
    _lib.check(rc, 'gen_rays')
    return rays8, mask


# ------------------------------------------------------------------ sample pipeline (section 2)
def bone_boxes(vol, nb):
    """int32[nb,6] = {x0,x1,y0,y1,z0,z1}: index box of the non-zero voxels of every bone's motion-weight channel."""
    boxes = torch.empty(nb, 6, device=vol.device, dtype=torch.int32)
    with _guard(vol):
        rc = _lib.lib().occnerf_bone_boxes(_chk(vol, torch.float32, 'vol'), int(nb), int(vol.shape[-1]), boxes.data_ptr(), _stream(vol))
    _lib.check(rc, 'bone_boxes')
    return boxes


def sample_warp(rays8, S, t_vals, Rs, Ts, vol, bbox_min, bbox_scale, t_rand=None, want_pts=False, boxes=None):
    """rays8[n,8] -> z_vals[n,S], x_skel[n*S,3], mask[n*S] (, pts[n*S,3]).  boxes (ops.bone_boxes of the same vol; render only:
    no jitter, no pts): bones that cannot reach a wave's samples are skipped, same bits."""
    n = rays8.shape[0]
    dev = rays8.device
    if boxes is not None and t_rand is None and not want_pts:
        z = torch.empty(n, S, device=dev, dtype=torch.float32)
        xs = torch.empty(n * S, 3, device=dev, dtype=torch.float32)
        mk = torch.empty(n * S, device=dev, dtype=torch.float32)
        _kmin, pmin = _host_f32(bbox_min, 3)
        _ksc, psc = _host_f32(bbox_scale, 3)
        with _guard_dev(dev):
            rc = _lib.lib().occnerf_sample_warp_culled(
                _chk(rays8, torch.float32, 'rays'), n, int(S), _chk(t_vals, torch.float32, 't_vals'),
                _chk(Rs, torch.float32, 'Rs'), _chk(Ts, torch.float32, 'Ts'), _chk(vol, torch.float32, 'vol'), int(Rs.shape[0]),
                int(vol.shape[-1]), _chk(boxes, torch.int32, 'boxes'), pmin, psc, z.data_ptr(), xs.data_ptr(), mk.data_ptr(),
                _stream(rays8))
        _lib.check(rc, 'sample_warp_culled')
        return z, xs, mk, None
    z = torch.empty(n, S, device=dev, dtype=torch.float32)
    xs = torch.empty(n * S, 3, device=dev, dtype=torch.float32)
    mk = torch.empty(n * S, device=dev, dtype=torch.float32)
    pts = torch.empty(n * S, 3, device=dev, dtype=torch.float32) if want_pts else None
    _kmin, pmin = _host_f32(bbox_min, 3)
    _ksc, psc = _host_f32(bbox_scale, 3)
    with _guard_dev(dev):
        rc = _lib.lib().occnerf_sample_warp(
            _chk(rays8, torch.float32, 'rays'), n, int(S), _chk(t_vals, torch.float32, 't_vals'),
            _opt(t_rand, torch.float32, 't_rand'), _chk(Rs, torch.float32, 'Rs'),
            _chk(Ts, torch.float32, 'Ts'), _chk(vol, torch.float32, 'vol'), int(Rs.shape[0]),
            int(vol.shape[-1]), pmin, psc, z.data_ptr(), None if pts is None else pts.data_ptr(),
            xs.data_ptr(), mk.data_ptr(), _stream(rays8))
    _lib.check(rc, 'sample_warp')
    return z, xs, mk, pts


def nonrigid_pack(weights, biases):
    dev = weights[0].device
    n = _lib.lib().occnerf_nonrigid_packed_floats()
    packed = torch.zeros(n, device=dev, dtype=torch.float32)
    with _guard_dev(dev):
        rc = _lib.lib().occnerf_nonrigid_pack(_ptr_table(weights, 'W'), _ptr_table(biases, 'b'),
                                              packed.data_ptr(), _stream(packed))
    _lib.check(rc, 'nonrigid_pack')
    return packed


def nonrigid(xyz, cond, hann, W0, b0, packed, out=None, direct=False):
    """direct=True: the 32-sample-wave direct-load kernel (cross-check / A-B timing)."""
    out = torch.empty_like(xyz) if out is None else out
    _kh, ph = _host_f32(hann, 6)
    fn = _lib.lib().occnerf_nonrigid_direct if direct else _lib.lib().occnerf_nonrigid
    with _guard(xyz):
        rc = fn(
            _chk(xyz, torch.float32, 'xyz'), xyz.shape[0], _chk(cond, torch.float32, 'cond'), ph,
            _chk(W0, torch.float32, 'W0'), _chk(b0, torch.float32, 'b0'),
            _chk(packed, torch.float32, 'packed'), _chk(out, torch.float32, 'xyz_out'), _stream(xyz))
    _lib.check(rc, 'nonrigid')
    return out


def nonrigid_rows(xyz, rows, count, cond, hann, W0, b0, packed):
    """Non-rigid offsets, in place, for the samples rows[0 .. count) only (list and count on the device)."""
    _kh, ph = _host_f32(hann, 6)
    with _guard(xyz):
        rc = _lib.lib().occnerf_nonrigid_rows(
            _chk(xyz, torch.float32, 'xyz'), rows.shape[0], _chk(rows, torch.int32, 'rows'),
            _chk(count, torch.int32, 'count'), _chk(cond, torch.float32, 'cond'), ph,
            _chk(W0, torch.float32, 'W0'), _chk(b0, torch.float32, 'b0'), _chk(packed, torch.float32, 'packed'),
            _stream(xyz))
    _lib.check(rc, 'nonrigid_rows')
    return xyz


def live_rows(mask):
    """-> rows int32[N] (first count entries valid: ascending indices with mask != 0), count int32[1]; no sync."""
    N = mask.shape[0]
    dev = mask.device
    nbytes = int(_lib.lib().occnerf_live_rows_temp_bytes(N))
    if nbytes < 0:
        raise RuntimeError('live_rows: temp size query failed')
    temp = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    rows = torch.empty(N, device=dev, dtype=torch.int32)
    count = torch.empty(1, device=dev, dtype=torch.int32)
    with _guard(mask):
        rc = _lib.lib().occnerf_live_rows(_chk(mask, torch.float32, 'mask'), N, rows.data_ptr(), count.data_ptr(),
                                          temp.data_ptr(), nbytes, _stream(mask))
    _lib.check(rc, 'live_rows')
    return rows, count


def scatter_raw(raw_c, rows, count, raw_full):
    with _guard(raw_c):
        rc = _lib.lib().occnerf_scatter_raw(_chk(raw_c, torch.float32, 'raw_c'), _chk(rows, torch.int32, 'rows'),
                                            _chk(count, torch.int32, 'count'), rows.shape[0],
                                            _chk(raw_full, torch.float32, 'raw_full'), _stream(raw_c))
    _lib.check(rc, 'scatter_raw')
    return raw_full


def center_classify(xyz, rows, count, geo, center, center_idx, center_agg, bound32, two_bound32, raw_c, flag=None):
    """Collapsed samples of the live list rows[0 .. count) (csrc/center.hip): flag uint8[len(rows)] -- 1 where the sample lies
    inside the radius of ops.knn_center's `center` AND its encoder input is bitwise the centre's (center_agg[36:40], ops.center_row):
    its whole feature row is then the centre's.  raw_c[o, 4] receives the signed distance of the flagged entries.
    geo: ops.point_pack's records.  Entries at and beyond count are left unwritten."""
    M = rows.shape[0]
    if flag is None:
        flag = torch.empty(M, device=xyz.device, dtype=torch.uint8)
    if flag.shape[0] < M or raw_c.shape[0] < M:
        raise RuntimeError('center_classify: flag and raw_c need a row per list entry')
    if center_idx.numel() < 10 or center_agg.numel() < 72 or center.numel() < 4:
        raise RuntimeError('center_classify: center[4], center_idx[>= 10] and center_agg[72] (ops.knn_center, ops.center_row)')
    with _guard(xyz):
        rc = _lib.lib().occnerf_center_classify(
            _chk(xyz, torch.float32, 'xyz'), _chk(rows, torch.int32, 'rows'), _chk(count, torch.int32, 'count'), M,
            _chk(geo, torch.float32, 'point_geo'), int(geo.shape[0]), _chk(center, torch.float32, 'center'),
            _chk(center_idx, torch.int32, 'center_idx'), _chk(center_agg, torch.float32, 'center_agg'),
            float(bound32), float(two_bound32), _chk(flag, torch.uint8, 'flag'), _chk(raw_c, torch.float32, 'raw_c'),
            _stream(xyz))
    _lib.check(rc, 'center_classify')
    return flag


def center_split(flag, rows, count, centre_row):
    """The live list without its flagged entries, order preserved (see the header) -> (keep int32[M], rows2 int32[M],
    count2 int32[1], in_rows int32[M], taken int32[1]): rows2 / count2 for the kNN and feature kernels, in_rows for the
    canonical MLP (a flagged entry reads row `centre_row` of its input), keep for center_merge_dist.  No sync."""
    M, dev = rows.shape[0], rows.device
    keep = torch.empty(M, device=dev, dtype=torch.int32)
    rows2 = torch.empty(M, device=dev, dtype=torch.int32)
    in_rows = torch.empty(M, device=dev, dtype=torch.int32)
    count2 = torch.empty(1, device=dev, dtype=torch.int32)
    taken = torch.empty(1, device=dev, dtype=torch.int32)
    if M == 0:
        count2.zero_()
        taken.zero_()
        return keep, rows2, count2, in_rows, taken
    nbytes = int(_lib.lib().occnerf_center_split_temp_bytes(M))
    if nbytes < 0:
        raise RuntimeError('center_split: temp size query failed')
    temp = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    with _guard(rows):
        rc = _lib.lib().occnerf_center_split(
            _chk(flag, torch.uint8, 'flag'), _chk(rows, torch.int32, 'rows'), _chk(count, torch.int32, 'count'), M,
            int(centre_row), keep.data_ptr(), rows2.data_ptr(), count2.data_ptr(), in_rows.data_ptr(), taken.data_ptr(),
            temp.data_ptr(), nbytes, _stream(rows))
    _lib.check(rc, 'center_split')
    return keep, rows2, count2, in_rows, taken


def center_merge_dist(raw2, keep, count2, raw_c):
    """raw_c[keep[o2], 4] = raw2[o2, 4] for o2 < count2: the kept entries' signed distance back at their list positions."""
    with _guard(raw2):
        rc = _lib.lib().occnerf_center_merge_dist(
            _chk(raw2, torch.float32, 'raw2'), _chk(keep, torch.int32, 'keep'), _chk(count2, torch.int32, 'count2'),
            keep.shape[0], _chk(raw_c, torch.float32, 'raw_c'), _stream(raw2))
    _lib.check(rc, 'center_merge_dist')
    return raw_c


def repeat_heads(keys, key_cols, count, rows=None, want_mask=False):
    """Run-length elimination of repeated samples (see the header): keys float32/int32 [M, C] (row-contiguous), the first
    key_cols columns compared as bit patterns; entry m is row rows[m] (rows given) or m, for m < count[0] (device).
    -> scan int32[cap], heads int32[cap], head_count int32[1], head_mask float32[M] or None; cap = len(rows) or M."""
    dev = keys.device
    if keys.dim() != 2 or not keys.is_contiguous() or keys.element_size() != 4:
        raise RuntimeError('repeat_heads: keys must be a contiguous [M, C] tensor of 4-byte elements')
    cap = keys.shape[0] if rows is None else rows.shape[0]
    scan = torch.empty(cap, device=dev, dtype=torch.int32)
    heads = torch.empty(cap, device=dev, dtype=torch.int32)
    head_count = torch.empty(1, device=dev, dtype=torch.int32)
    head_mask = torch.zeros(keys.shape[0], device=dev, dtype=torch.float32) if want_mask else None
    if cap == 0:
        head_count.zero_()
        return scan, heads, head_count, head_mask
    nbytes = int(_lib.lib().occnerf_repeat_heads_temp_bytes(cap))
    if nbytes < 0:
        raise RuntimeError('repeat_heads: temp size query failed')
    temp = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    with _guard_dev(dev):
        rc = _lib.lib().occnerf_repeat_heads(
            keys.data_ptr(), keys.shape[1], int(key_cols), _opt(rows, torch.int32, 'rows'),
            _chk(count, torch.int32, 'count'), cap, scan.data_ptr(), heads.data_ptr(), head_count.data_ptr(),
            None if head_mask is None else head_mask.data_ptr(), temp.data_ptr(), nbytes, _stream(keys))
    _lib.check(rc, 'repeat_heads')
    return scan, heads, head_count, head_mask


def unique_heads(keys, key_cols, heads, count, scan=None, scan_count=None):
    """Distinct entries of a list (see the header): heads int32[cap] (or None: entry j is row j of keys, cap = rows of
    keys), count int32[1] on the device -> (heads_out int32[cap], count_out int32[1]); scan (optional, with scan_count) is
    rewritten in place from 1-based entry numbers to 1-based positions in heads_out."""
    dev = keys.device
    if keys.dim() != 2 or not keys.is_contiguous() or keys.element_size() != 4:
        raise RuntimeError('unique_heads: keys must be a contiguous [M, C] tensor of 4-byte elements')
    cap = keys.shape[0] if heads is None else heads.shape[0]
    heads_out = torch.empty(cap, device=dev, dtype=torch.int32)
    count_out = torch.empty(1, device=dev, dtype=torch.int32)
    if cap == 0:
        count_out.zero_()
        return heads_out, count_out
    nbytes = int(_lib.lib().occnerf_unique_heads_temp_bytes(cap))
    if nbytes <= 0:
        raise RuntimeError('unique_heads: temp size query failed')
    temp = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    with _guard_dev(dev):
        rc = _lib.lib().occnerf_unique_heads(
            keys.data_ptr(), keys.shape[1], int(key_cols), _opt(heads, torch.int32, 'heads'),
            _chk(count, torch.int32, 'count'), cap, heads_out.data_ptr(), count_out.data_ptr(),
            _opt(scan, torch.int32, 'scan'), _opt(scan_count, torch.int32, 'scan_count'),
            0 if scan is None else scan.shape[0], temp.data_ptr(), nbytes, _stream(keys))
    _lib.check(rc, 'unique_heads')
    return heads_out, count_out


def scatter_raw_heads(raw_h, raw_c, rows, count, scan_a, scan_b, raw_full):
    with _guard(raw_c):
        rc = _lib.lib().occnerf_scatter_raw_heads(
            _chk(raw_h, torch.float32, 'raw_h'), _chk(raw_c, torch.float32, 'raw_c'), _chk(rows, torch.int32, 'rows'),
            _chk(count, torch.int32, 'count'), _opt(scan_a, torch.int32, 'scan_a'), _opt(scan_b, torch.int32, 'scan_b'),
            rows.shape[0], _chk(raw_full, torch.float32, 'raw_full'), _stream(raw_c))
    _lib.check(rc, 'scatter_raw_heads')
    return raw_full


def nonrigid_pack_bf16(weights):
    dev = weights[0].device
    n = _lib.lib().occnerf_nonrigid_packed_bf16_bytes()
    packed = torch.zeros(n // 2, device=dev, dtype=torch.bfloat16)
    with _guard_dev(dev):
        rc = _lib.lib().occnerf_nonrigid_pack_bf16(_ptr_table(weights[:6], 'W'), packed.data_ptr(), _stream(packed))
    _lib.check(rc, 'nonrigid_pack_bf16')
    return packed


def nonrigid_pack_f16(weights):
    """Split-fp16 operand stream of the non-rigid MLP (cfg.mlp_precision = 'f16x3': csrc/split.h F16x3)."""
    dev = weights[0].device
    n = _lib.lib().occnerf_nonrigid_packed_bf16_bytes()               # same layout, 2-byte elements
    packed = torch.zeros(n // 2, device=dev, dtype=torch.float16)
    with _guard_dev(dev):
        rc = _lib.lib().occnerf_nonrigid_pack_f16(_ptr_table(weights[:6], 'W'), packed.data_ptr(), _stream(packed))
    _lib.check(rc, 'nonrigid_pack_f16')
    return packed


def _nonrigid_f16x3(xyz, rows, count, cond, hann, W0, b0, packed, packed_f16, out, domain_flag=None):
    _kh, ph = _host_f32(hann, 6)
    n_max = xyz.shape[0] if rows is None else rows.shape[0]
    with _guard(xyz):
        rc = _lib.lib().occnerf_nonrigid_f16x3(
            _chk(xyz, torch.float32, 'xyz'), n_max, _opt(rows, torch.int32, 'rows'), _opt(count, torch.int32, 'count'),
            _chk(cond, torch.float32, 'cond'), ph, _chk(W0, torch.float32, 'W0'), _chk(b0, torch.float32, 'b0'),
            _chk(packed, torch.float32, 'packed'), _chk(packed_f16, torch.float16, 'packed_f16'),
            _chk(out, torch.float32, 'xyz_out'), _opt(domain_flag, torch.int32, 'domain_flag'), _stream(xyz))
    _lib.check(rc, 'nonrigid_f16x3')
    return out


def nonrigid_bf16x3(xyz, cond, hann, W0, b0, packed, packed_bf16, out=None, domain_flag=None):
    """Split-operand non-rigid MLP; the dtype of the packed stream selects the split (bfloat16: bf16x3, float16: f16x3).
    domain_flag (int32[1] on the device, f16x3 only): bit 0 is set when a hidden activation reached the mode's clamp (4 094)."""
    out = torch.empty_like(xyz) if out is None else out
    if packed_bf16.dtype == torch.float16:
        return _nonrigid_f16x3(xyz, None, None, cond, hann, W0, b0, packed, packed_bf16, out, domain_flag)
    _kh, ph = _host_f32(hann, 6)
    with _guard(xyz):
        rc = _lib.lib().occnerf_nonrigid_bf16x3(
            _chk(xyz, torch.float32, 'xyz'), xyz.shape[0], _chk(cond, torch.float32, 'cond'), ph,
            _chk(W0, torch.float32, 'W0'), _chk(b0, torch.float32, 'b0'), _chk(packed, torch.float32, 'packed'),
            _chk(packed_bf16, torch.bfloat16, 'packed_bf16'), _chk(out, torch.float32, 'xyz_out'), _stream(xyz))
    _lib.check(rc, 'nonrigid_bf16x3')
    return out


def nonrigid_bf16x3_rows(xyz, rows, count, cond, hann, W0, b0, packed, packed_bf16, domain_flag=None):
    """In place on the listed samples (the split-operand counterpart of nonrigid_rows): xyz[rows[i]] += offset, i < count[0]."""
    if packed_bf16.dtype == torch.float16:
        return _nonrigid_f16x3(xyz, rows, count, cond, hann, W0, b0, packed, packed_bf16, xyz, domain_flag)
    _kh, ph = _host_f32(hann, 6)
    with _guard(xyz):
        rc = _lib.lib().occnerf_nonrigid_bf16x3_rows(
            _chk(xyz, torch.float32, 'xyz'), rows.shape[0], _chk(rows, torch.int32, 'rows'), _chk(count, torch.int32, 'count'),
            _chk(cond, torch.float32, 'cond'), ph, _chk(W0, torch.float32, 'W0'), _chk(b0, torch.float32, 'b0'),
            _chk(packed, torch.float32, 'packed'), _chk(packed_bf16, torch.bfloat16, 'packed_bf16'), _stream(xyz))
    _lib.check(rc, 'nonrigid_bf16x3_rows')
    return xyz


def msknn(xyz, points, index_map, scale_begin, seed_from_coarser):
    N = xyz.shape[0]
    nscale = len(scale_begin) - 1
    out = torch.empty(N, nscale, 10, device=xyz.device, dtype=torch.int32)
    _kb, pb = _host_i32(scale_begin)
    _ks, ps = _host_i32(seed_from_coarser)
    with _guard(xyz):
        rc = _lib.lib().occnerf_msknn(_chk(xyz, torch.float32, 'xyz'), N,
                                      _chk(points, torch.float32, 'points'),
                                      _chk(index_map, torch.int32, 'index_map'), pb, ps, nscale,
                                      out.data_ptr(), _stream(xyz))
    _lib.check(rc, 'msknn')
    return out


def knn_center(c, points, index_map, scale_begin):
    """c[3] (device) against the brute-force multi-scale layout (ops.msknn's points / index_map / scale_begin) ->
    (center[4] = (c, r^2), idx[nscale, 10]): c's neighbours and the squared radius inside which every query provably has the same
    neighbours in the same order (0: no such radius).  For msknn_clustered(center=...)."""
    nscale = len(scale_begin) - 1
    center = torch.empty(4, device=c.device, dtype=torch.float32)
    idx = torch.empty(nscale, 10, device=c.device, dtype=torch.int32)
    _kb, pb = _host_i32(scale_begin)
    with _guard(c):
        rc = _lib.lib().occnerf_knn_center(_chk(c, torch.float32, 'c'), _chk(points, torch.float32, 'points'),
                                           _chk(index_map, torch.int32, 'index_map'), pb, nscale, center.data_ptr(), idx.data_ptr(),
                                           _stream(c))
    _lib.check(rc, 'knn_center')
    return center, idx


def msknn_clustered(xyz, n_rays, S, cl, seed_from_coarser, mask=None, rows=None, count=None, out=None, center=None):
    """cl: device-side cluster layout (dict, see Network._context / geometry.build_knn_clusters).
    mask[n_rays*S] (optional): samples with mask == 0 are skipped, their output rows left unwritten.
    rows / count (optional, instead of mask): ascending int32 list of the samples to query and its length on the device.
    center (optional): ops.knn_center's pair -- queries inside its radius take the cached indices (same results)."""
    nscale = int(cl['ranges'].shape[0]) + 1
    if out is None:
        out = torch.empty(n_rays * S, nscale, 10, device=xyz.device, dtype=torch.int32)
    if (rows is None) != (count is None) or (rows is not None and mask is not None):
        raise RuntimeError('msknn_clustered: rows and count come together, instead of mask')
    ray_start = torch.empty(n_rays + 1, device=xyz.device, dtype=torch.int32) if rows is not None else None
    _kc, pc = _host_i32(cl['coarse_rows'])
    _ks, ps = _host_i32(seed_from_coarser)
    with _guard(xyz):
        rc = _lib.lib().occnerf_msknn_clustered_centered(
            _chk(xyz, torch.float32, 'xyz'), _opt(mask, torch.float32, 'mask'), int(n_rays), int(S),
            _chk(cl['points'], torch.float32, 'points'), _chk(cl['centers'], torch.float32, 'centers'), _chk(cl['ranges'], torch.int32, 'cluster_ranges'),
            _chk(cl['radius'], torch.float32, 'cluster_radius'), int(cl['ncl']),
            _opt(cl.get('group_centers'), torch.float32, 'group_centers'), _opt(cl.get('group_ranges'), torch.int32, 'group_ranges'),
            _opt(cl.get('group_radius'), torch.float32, 'group_radius'), int(cl.get('ngrp', 0)), pc, ps, nscale,
            _opt(rows, torch.int32, 'rows'), _opt(count, torch.int32, 'count'),
            None if ray_start is None else ray_start.data_ptr(),
            None if center is None else _chk(center[0], torch.float32, 'center'),
            None if center is None else _chk(center[1], torch.int32, 'center_idx'), out.data_ptr(), _stream(xyz))
    _lib.check(rc, 'msknn_clustered')
    return out


def knn_small(q, s, k):
    out = torch.empty(q.shape[0], k, device=q.device, dtype=torch.int32)
    with _guard(q):
        rc = _lib.lib().occnerf_knn_small(_chk(q, torch.float32, 'q'), q.shape[0],
                                          _chk(s, torch.float32, 's'), s.shape[0], int(k),
                                          out.data_ptr(), _stream(q))
    _lib.check(rc, 'knn_small')
    return out


def unit_normals(normals):
    out = torch.empty_like(normals)
    with _guard(normals):
        rc = _lib.lib().occnerf_unit_normals(_chk(normals, torch.float64, 'normals'), normals.shape[0],
                                             out.data_ptr(), _stream(normals))
    _lib.check(rc, 'unit_normals')
    return out


def point_sdf(point_cloud, point_base, normals, unit, kidx):
    P = point_cloud.shape[0]
    kb = torch.empty(P, 3, device=point_cloud.device, dtype=torch.float64)
    dist = torch.empty(P, device=point_cloud.device, dtype=torch.float32)
    with _guard(point_cloud):
        rc = _lib.lib().occnerf_point_sdf(
            _chk(point_cloud, torch.float32, 'point_cloud'), _chk(point_base, torch.float32, 'point_base'),
            _chk(normals, torch.float64, 'normals'), _chk(unit, torch.float64, 'unit_normals'),
            _chk(kidx, torch.int32, 'kidx'), P, kb.data_ptr(), dist.data_ptr(), _stream(point_cloud))
    _lib.check(rc, 'point_sdf')
    return kb, dist


def table_stride():
    """Row pitch (floats) of the per-point feature table."""
    return int(_lib.lib().occnerf_point_table_stride())


def point_table(knn_base, sdf, learnable, bound32, two_bound32, embeddings, offsets, S, H):
    P = knn_base.shape[0]
    table = torch.empty(P, table_stride(), device=knn_base.device, dtype=torch.float32)
    with _guard(knn_base):
        rc = _lib.lib().occnerf_point_table(
            _chk(knn_base, torch.float64, 'knn_base'), _chk(sdf, torch.float32, 'point_sdf'),
            _chk(learnable, torch.float32, 'learnable'), P, float(bound32), float(two_bound32),
            _chk(embeddings, torch.float32, 'embeddings'), _chk(offsets, torch.int32, 'offsets'),
            _host_offsets(offsets), int(offsets.shape[0] - 1), float(S), int(H), table.data_ptr(),
            _stream(knn_base))
    _lib.check(rc, 'point_table')
    return table


def point_pack(point_base, normals, unit, counter, table):
    """Per-point records of the 8-lanes-per-sample feature kernel: (geo[P,16], tail[P,4]) -- see the header."""
    P, dev = point_base.shape[0], point_base.device
    geo = torch.empty(P, 16, device=dev, dtype=torch.float32)
    tail = torch.empty(P, 4, device=dev, dtype=torch.float32)
    with _guard_dev(dev):
        rc = _lib.lib().occnerf_point_pack(
            _chk(point_base, torch.float32, 'point_base'), _chk(normals, torch.float64, 'normals'),
            _chk(unit, torch.float64, 'unit_normals'), _chk(counter, torch.float32, 'counter'),
            _chk(table, torch.float32, 'table'), P, geo.data_ptr(), tail.data_ptr(), _stream(point_base))
    _lib.check(rc, 'point_pack')
    return geo, tail


def center_row(mlp_in_row, enc_in_row):
    """The 72 floats sample_features(center_agg=...) takes: [columns 0..35 of the centre sample's mlp_in | its encoder input x[4] |
    its columns 36..67 (the 32 encoded features of x)]."""
    return torch.cat([mlp_in_row[:36], enc_in_row[:4], mlp_in_row[36:68]]).contiguous()


def sample_features(xyz, knn_idxs, point_base, normals, unit, counter, table, bound32, two_bound32,
                    embeddings, offsets, S, H, raw=None, want_enc_in=False, geo_idxs=None,
                    att_in=None, rows=None, count=None, pack=None, center=None, center_agg=None, mlp_in_out=None):
    """rows (int32[M], optional): compact list of samples to evaluate; outputs then have M rows.
    mlp_in_out (float32[>= M, 68], optional): the buffer the feature rows are written to, and returned as mlp_in, instead of a
    fresh [M, 68] one (a caller that keeps further rows behind them: Network's centre row).
    center / center_agg (optional, renderer's path): ops.knn_center's [4] and ops.center_row of a sample with the centre's
    neighbour lists -- groups of samples inside the radius copy its aggregate columns instead of gathering rows, and its encoded
    columns too when their encoder input is bitwise the centre's (same bits).  FRESHNESS CONTRACT (not checkable here):
    `center` must come from ops.knn_center on the SAME point set the kNN indices were searched in, and `center_agg` from this
    function on a sample at that centre with the SAME table, counter, embeddings and pack -- stale ones give silently wrong
    features.  Network computes both once per frame from the frame's own table (`_knn_center`) and checks the table's
    identity and version before every use (`_render_rays`).
    count (int32[1] on the device, optional, with rows): the list's real length; M is then a capacity.
    pack: point_pack(...) of the same per-point inputs (built here when the renderer's kernel applies and the caller
    did not cache it)."""
    N = xyz.shape[0] if rows is None else rows.shape[0]
    dev = xyz.device
    if (pack is None and N > 0 and knn_idxs.shape[1] == 4 and geo_idxs is None and att_in is None
            and counter is not None and table.dim() == 2 and table.shape[1] == table_stride()):
        pack = point_pack(point_base, normals, unit, counter, table)
    geo, tail = pack if pack is not None else (None, None)
    if table.dim() != 2 or table.shape[1] != table_stride():
        raise RuntimeError(f'sample_features: table must be [P,{table_stride()}] (ops.point_table), got {tuple(table.shape)}')
    if mlp_in_out is None:
        mlp_in = torch.empty(N, 68, device=dev, dtype=torch.float32)
    else:
        mlp_in = mlp_in_out
        if mlp_in.dim() != 2 or mlp_in.shape[0] < N or mlp_in.shape[1] != 68:
            raise RuntimeError(f'sample_features: mlp_in_out must be [>= {N}, 68], got {tuple(mlp_in.shape)}')
    raw = torch.empty(N, 5, device=dev, dtype=torch.float32) if raw is None else raw
    enc_in = torch.empty(N, 4, device=dev, dtype=torch.float32) if want_enc_in else None
    with _guard_dev(dev):
        rc = _lib.lib().occnerf_sample_features_centered(
            _chk(xyz, torch.float32, 'xyz'), N, _chk(knn_idxs, torch.int32, 'knn_idxs'),
            int(knn_idxs.shape[1]), _chk(point_base, torch.float32, 'point_base'),
            _chk(normals, torch.float64, 'normals'), _chk(unit, torch.float64, 'unit_normals'),
            _opt(counter, torch.float32, 'counter'), _chk(table, torch.float32, 'table'),
            float(bound32), float(two_bound32), _chk(embeddings, torch.float32, 'embeddings'),
            _chk(offsets, torch.int32, 'offsets'), _host_offsets(offsets), int(offsets.shape[0] - 1),
            float(S), int(H), _opt(geo_idxs, torch.int32, 'geo_idxs'), _opt(att_in, torch.float32, 'att_in'),
            _opt(rows, torch.int32, 'rows'), _opt(count, torch.int32, 'count'),
            _opt(geo, torch.float32, 'point_geo'), _opt(tail, torch.float32, 'point_tail'),
            0 if geo is None else int(geo.shape[0]),
            _opt(center, torch.float32, 'center'), _opt(center_agg, torch.float32, 'center_agg'),
            _chk(mlp_in, torch.float32, 'mlp_in'), _chk(raw, torch.float32, 'raw'),
            None if enc_in is None else enc_in.data_ptr(), _stream(xyz))
    _lib.check(rc, 'sample_features')
    return mlp_in, raw, enc_in


def canonical_mlp_pack(weights, biases):
    """weights/biases: the 10 Linear layers in module order (see the header)."""
    dev = weights[0].device
    n = _lib.lib().occnerf_canonical_mlp_packed_floats()
    packed = torch.zeros(n, device=dev, dtype=torch.float32)
    with _guard_dev(dev):
        rc = _lib.lib().occnerf_canonical_mlp_pack(_ptr_table(weights, 'W'), _ptr_table(biases, 'b'),
                                                   packed.data_ptr(), _stream(packed))
    _lib.check(rc, 'canonical_mlp_pack')
    return packed


def canonical_mlp(mlp_in, packed, raw, direct=False, count=None, in_rows=None):
    """fp32 MLP trunks.  direct=True: the 32-sample-wave direct-load kernel (cross-check / A-B timing).
    count (int32[1] on the device): only the first count rows exist; the host does not know the number.
    in_rows (int32, with count): output row n is computed from input row in_rows[n]."""
    if in_rows is not None:
        with _guard(mlp_in):
            rc = _lib.lib().occnerf_canonical_mlp_rows(
                _chk(mlp_in, torch.float32, 'mlp_in'), _chk(in_rows, torch.int32, 'in_rows'), in_rows.shape[0],
                _chk(count, torch.int32, 'count'), _chk(packed, torch.float32, 'packed'),
                _chk(raw, torch.float32, 'raw'), _stream(mlp_in))
        _lib.check(rc, 'canonical_mlp_rows')
        return raw
    if count is not None:
        with _guard(mlp_in):
            rc = _lib.lib().occnerf_canonical_mlp_counted(
                _chk(mlp_in, torch.float32, 'mlp_in'), mlp_in.shape[0], _chk(count, torch.int32, 'count'),
                _chk(packed, torch.float32, 'packed'), _chk(raw, torch.float32, 'raw'), _stream(mlp_in))
        _lib.check(rc, 'canonical_mlp_counted')
        return raw
    fn = _lib.lib().occnerf_canonical_mlp_direct if direct else _lib.lib().occnerf_canonical_mlp
    with _guard(mlp_in):
        rc = fn(_chk(mlp_in, torch.float32, 'mlp_in'), mlp_in.shape[0], _chk(packed, torch.float32, 'packed'),
                _chk(raw, torch.float32, 'raw'), _stream(mlp_in))
    _lib.check(rc, 'canonical_mlp')
    return raw


def trunks_pack_bf16(weights, out=None):
    """Plain-bf16 operand stream of the nine MFMA layers for the training step's fused forward (csrc/trunks.hip)."""
    dev = weights[0].device
    if out is None:
        out = torch.zeros(_lib.lib().occnerf_trunks_packed_bytes() // 2, device=dev, dtype=torch.bfloat16)
    with _guard_dev(dev):
        rc = _lib.lib().occnerf_trunks_pack_bf16(_ptr_table(weights[:9], 'W'), out.data_ptr(), _stream(out))
    _lib.check(rc, 'trunks_pack_bf16')
    return out


def trunks_forward_bf16(agg, var, enc, packed_f32, packed_bf16):
    """Both trunks forward in one kernel, the activations the backward needs written on the way (csrc/trunks.hip).
    -> X0[M,96], [A1..A4][M,256], GEO[M,96], [B1..B4][M,256] (bf16, row-major), raw4[M,4] fp32."""
    M, dev, bf = agg.shape[0], agg.device, torch.bfloat16
    X0 = torch.empty(M, 96, device=dev, dtype=bf)
    A = [torch.empty(M, 256, device=dev, dtype=bf) for _ in range(4)]
    GEO = torch.empty(M, 96, device=dev, dtype=bf)
    B = [torch.empty(M, 256, device=dev, dtype=bf) for _ in range(4)]
    raw4 = torch.empty(M, 4, device=dev, dtype=torch.float32)
    pa = (C.c_void_p * 4)(*[t.data_ptr() for t in A])
    pb = (C.c_void_p * 4)(*[t.data_ptr() for t in B])
    with _guard(agg):
        rc = _lib.lib().occnerf_trunks_forward_bf16(
            _chk(agg, torch.float32, 'agg'), _chk(var, torch.float32, 'var'), _chk(enc, torch.float32, 'enc'), M,
            _chk(packed_f32, torch.float32, 'packed_f32'), _chk(packed_bf16, torch.bfloat16, 'packed_bf16'), X0.data_ptr(), pa,
            GEO.data_ptr(), pb, raw4.data_ptr(), _stream(agg))
    _lib.check(rc, 'trunks_forward_bf16')
    return X0, A, GEO, B, raw4


def canonical_mlp_pack_bf16(weights):
    """hi/lo bf16 split of the 10 weight matrices in bf16-MFMA operand order."""
    dev = weights[0].device
    n = _lib.lib().occnerf_canonical_mlp_packed_bf16_bytes()
    packed = torch.zeros(n // 2, device=dev, dtype=torch.bfloat16)
    with _guard_dev(dev):
        rc = _lib.lib().occnerf_canonical_mlp_pack_bf16(_ptr_table(weights, 'W'), packed.data_ptr(),
                                                        _stream(packed))
    _lib.check(rc, 'canonical_mlp_pack_bf16')
    return packed


def canonical_mlp_pack_f16(weights):
    """Split-fp16 operand stream of the canonical MLP (cfg.mlp_precision = 'f16x3': csrc/split.h F16x3): Wh = f16(W),
    Wl' = f16((W - Wh) 2^11), in fp16-MFMA operand order."""
    dev = weights[0].device
    n = _lib.lib().occnerf_canonical_mlp_packed_bf16_bytes()          # same layout, 2-byte elements
    packed = torch.zeros(n // 2, device=dev, dtype=torch.float16)
    with _guard_dev(dev):
        rc = _lib.lib().occnerf_canonical_mlp_pack_f16(_ptr_table(weights, 'W'), packed.data_ptr(), _stream(packed))
    _lib.check(rc, 'canonical_mlp_pack_f16')
    return packed


def canonical_mlp_bf16x3(mlp_in, packed, packed_bf16, raw, variant=0, count=None, in_rows=None, domain_flag=None):
    """Split-operand canonical MLP; the dtype of the packed stream selects the split (bfloat16: bf16x3, float16: f16x3).
    count (int32[1] on the device): entries to evaluate, read by the kernel (the launch covers the worst case);
    in_rows (int32, optional): entry n takes input row in_rows[n]; results are compact (raw[n]).
    domain_flag (int32[1] on the device, f16x3 only): bit 0 is set when a value reached the mode's clamp (csrc/split.h)."""
    if packed_bf16.dtype == torch.float16:
        n_max = mlp_in.shape[0] if in_rows is None else in_rows.shape[0]
        with _guard(mlp_in):
            rc = _lib.lib().occnerf_canonical_mlp_f16x3(
                _chk(mlp_in, torch.float32, 'mlp_in'), _opt(in_rows, torch.int32, 'in_rows'), n_max,
                _opt(count, torch.int32, 'count'), _chk(packed, torch.float32, 'packed'),
                _chk(packed_bf16, torch.float16, 'packed_f16'), _chk(raw, torch.float32, 'raw'),
                _opt(domain_flag, torch.int32, 'domain_flag'), _stream(mlp_in))
        _lib.check(rc, 'canonical_mlp_f16x3')
        return raw
    with _guard(mlp_in):
        if count is None:
            assert in_rows is None
            rc = _lib.lib().occnerf_canonical_mlp_bf16x3(
                _chk(mlp_in, torch.float32, 'mlp_in'), mlp_in.shape[0], _chk(packed, torch.float32, 'packed'),
                _chk(packed_bf16, torch.bfloat16, 'packed_bf16'), _chk(raw, torch.float32, 'raw'),
                int(variant), _stream(mlp_in))
        else:
            n_max = mlp_in.shape[0] if in_rows is None else in_rows.shape[0]
            rc = _lib.lib().occnerf_canonical_mlp_bf16x3_rows(
                _chk(mlp_in, torch.float32, 'mlp_in'), _opt(in_rows, torch.int32, 'in_rows'), n_max,
                _chk(count, torch.int32, 'count'), _chk(packed, torch.float32, 'packed'),
                _chk(packed_bf16, torch.bfloat16, 'packed_bf16'), _chk(raw, torch.float32, 'raw'), int(variant),
                _stream(mlp_in))
    _lib.check(rc, 'canonical_mlp_bf16x3')
    return raw


def composite(raw, mask, z_vals, rays8, bgcolor, want_weights=False, want_term=False, out=None, out_rows=None):
    """out_rows (int64[n], optional): results of ray r are written to row out_rows[r] of `out` = (rgb, acc, depth)
    (caller-allocated, at least max(out_rows)+1 rows; without out_rows: exactly n rows)."""
    n, S = z_vals.shape
    dev = raw.device
    if out is None:
        if out_rows is not None:
            raise RuntimeError('composite: out_rows needs caller-allocated outputs')
        out = (torch.empty(n, 3, device=dev, dtype=torch.float32), torch.empty(n, device=dev, dtype=torch.float32),
               torch.empty(n, device=dev, dtype=torch.float32))
    rgb, acc, dep = out
    for t, nm in ((rgb, 'rgb'), (acc, 'acc'), (dep, 'depth')):
        _chk(t, torch.float32, nm)
    w = torch.empty(n, S, device=dev, dtype=torch.float32) if want_weights else None
    tp = torch.empty(n, device=dev, dtype=torch.int32) if want_term else None
    _kbg, pbg = _host_f32(bgcolor, 3)
    with _guard_dev(dev):
        rc = _lib.lib().occnerf_composite(
            _chk(raw, torch.float32, 'raw'), _chk(mask, torch.float32, 'mask'),
            _chk(z_vals, torch.float32, 'z_vals'), _chk(rays8, torch.float32, 'rays'), pbg, n, int(S),
            rgb.data_ptr(), acc.data_ptr(), dep.data_ptr(), None if w is None else w.data_ptr(),
            None if tp is None else tp.data_ptr(), _opt(out_rows, torch.int64, 'out_rows'), _stream(raw))
    _lib.check(rc, 'composite')
    return rgb, acc, dep, w, tp


# ------------------------------------------------------------------ per-frame preamble
def pose_motion_bases(pose_decoder, posevec, refine, dst_Rs, dst_Ts, cnl_gtfms):
    """a2 + a3 in one launch -> Rs[24,3,3], Ts[24,3] (float32, on the device)."""
    import torch.nn as nn
    dev = dst_Rs.device
    lin = [m for m in pose_decoder.block_mlps if isinstance(m, nn.Linear)]
    if len(lin) != 5 or lin[0].in_features != 69 or lin[0].out_features != 256 or lin[4].out_features != 69:
        raise RuntimeError('pose_motion_bases: the fused kernel is built for the 69 -> 256 x4 -> 69 refiner of occnerf.yaml')
    Rs = torch.empty(24, 3, 3, device=dev, dtype=torch.float32)
    Ts = torch.empty(24, 3, device=dev, dtype=torch.float32)
    with _guard_dev(dev):
        rc = _lib.lib().occnerf_pose_motion_bases(
            _ptr_table([m.weight.detach() for m in lin], 'W'), _ptr_table([m.bias.detach() for m in lin], 'b'),
            _chk(posevec, torch.float32, 'posevec'), int(bool(refine)), _chk(dst_Rs, torch.float32, 'dst_Rs'),
            _chk(dst_Ts, torch.float32, 'dst_Ts'), _chk(cnl_gtfms, torch.float32, 'cnl_gtfms'), Rs.data_ptr(),
            Ts.data_ptr(), _stream(dst_Rs))
    _lib.check(rc, 'pose_motion_bases')
    return Rs, Ts


def prior_softmax(decoded, prior):
    """softmax over channels of decoded[C,...] + log(prior[C,...]) -> vol, same shape."""
    Cn = decoded.shape[0]
    V = decoded.numel() // Cn
    vol = torch.empty_like(decoded)
    with _guard(decoded):
        rc = _lib.lib().occnerf_prior_softmax(_chk(decoded, torch.float32, 'decoded'), _chk(prior, torch.float32, 'prior'),
                                              int(Cn), int(V), vol.data_ptr(), _stream(decoded))
    _lib.check(rc, 'prior_softmax')
    return vol


def ray_order(dirs):
    """dirs: [R,3] float32 GPU tensor (any row stride, unit element stride: a slice of rays8 works) -> int64[R], the Morton
    walk of the rays (csrc/rays.hip; occnerf_amd/rayorder.py is the same construction in torch ops).  No sync."""
    R = dirs.shape[0]
    order = torch.empty(R, device=dirs.device, dtype=torch.int64)
    if R == 0:
        return order
    if not dirs.is_cuda or dirs.dtype != torch.float32 or dirs.dim() != 2 or dirs.shape[1] != 3 or dirs.stride(1) != 1:
        raise RuntimeError('ray_order: dirs must be a float32 [R,3] GPU tensor with unit element stride')
    nbytes = int(_lib.lib().occnerf_ray_order_temp_bytes(R))
    if nbytes < 0:
        raise RuntimeError('ray_order: temp size query failed')
    temp = torch.empty(nbytes, device=dirs.device, dtype=torch.uint8)
    with _guard(dirs):
        rc = _lib.lib().occnerf_ray_order(dirs.data_ptr(), R, int(dirs.stride(0)), order.data_ptr(), temp.data_ptr(), nbytes,
                                          _stream(dirs))
    _lib.check(rc, 'ray_order')
    return order


def pack_rays(rays, near, far, order=None):
    """rays[2,R,3], near[R,1], far[R,1] -> rays8[R,8] in `order` (int64 permutation, optional)."""
    R = rays.shape[1]
    rays8 = torch.empty(R, 8, device=rays.device, dtype=torch.float32)
    with _guard(rays):
        rc = _lib.lib().occnerf_pack_rays(_chk(rays, torch.float32, 'rays'), _chk(near, torch.float32, 'near'),
                                          _chk(far, torch.float32, 'far'), _opt(order, torch.int64, 'order'), R,
                                          rays8.data_ptr(), _stream(rays))
    _lib.check(rc, 'pack_rays')
    return rays8


# ------------------------------------------------------------------ training path: neighbour aggregation
def agg_forward(feats, knn, atts):
    """agg[n] = sum_j atts[n,j] * feats[knn[n,j]]  (feats[P,F] fp32, knn[N,K] int32, atts[N,K] fp32)."""
    N, K = knn.shape
    F = feats.shape[1]
    agg = torch.empty(N, F, device=feats.device, dtype=torch.float32)
    with _guard(feats):
        rc = _lib.lib().occnerf_agg_forward(_chk(feats, torch.float32, 'feats'), int(F), _chk(knn, torch.int32, 'knn'),
                                            _chk(atts, torch.float32, 'atts'), N, int(K), agg.data_ptr(), _stream(feats))
    _lib.check(rc, 'agg_forward')
    return agg


def agg_backward(grad_agg, knn, atts, P):
    N, K = knn.shape
    F = grad_agg.shape[1]
    W = int(_lib.lib().occnerf_agg_backward_slices(N))
    partial = torch.empty(W, P, F, device=grad_agg.device, dtype=torch.float32)
    nbytes = int(_lib.lib().occnerf_agg_backward_scratch_bytes(N, int(F)))
    scratch = torch.empty(max(nbytes, 16), device=grad_agg.device, dtype=torch.uint8)
    with _guard(grad_agg):
        rc = _lib.lib().occnerf_agg_backward(_chk(grad_agg, torch.float32, 'grad_agg'), int(F),
                                             _chk(knn, torch.int32, 'knn'), _chk(atts, torch.float32, 'atts'), N,
                                             int(K), int(P), partial.data_ptr(), scratch.data_ptr(), nbytes,
                                             _stream(grad_agg))
    _lib.check(rc, 'agg_backward')
    return partial.sum(0)


class _Aggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, knn, atts):
        feats = feats.contiguous()
        ctx.save_for_backward(knn, atts)
        ctx.P = feats.shape[0]
        return agg_forward(feats, knn, atts)

    @staticmethod
    def backward(ctx, grad_agg):
        knn, atts = ctx.saved_tensors
        return agg_backward(grad_agg.contiguous(), knn, atts, ctx.P), None, None


def aggregate(feats, knn, atts):
    """Differentiable (w.r.t. feats) weighted neighbour sum; knn and atts carry no gradient.  Runs of consecutive samples whose
    ids AND weights are bitwise identical are evaluated / scattered once (exact for arbitrary atts).  Limits of the backward,
    refused by name: K <= 64 neighbours, F <= 64 columns, P <= 32 x min(1024, 18432 // F) rows (16 832 at F = 35)."""
    return _Aggregate.apply(feats, knn.contiguous(), atts.contiguous())


# ------------------------------------------------------------------ LPIPS (VGG16, v0.1) and the patch images of the batch
def lpips_pack(conv_w, conv_b, lins, shift, scale):
    """13 conv weights [Cout,Cin,3,3] / biases, 5 lin weights [1,C,1,1], the scaling layer's shift / scale -> the packed blob
    of occnerf_lpips_forward / _backward (forward and data-gradient operand layouts)."""
    dev = conv_w[0].device
    packed = torch.empty(int(_lib.lib().occnerf_lpips_packed_floats()), device=dev, dtype=torch.float32)
    w = [t.detach().contiguous() for t in conv_w]
    b = [t.detach().contiguous() for t in conv_b]
    li = [t.detach().contiguous() for t in lins]
    sh, sc = shift.detach().contiguous(), scale.detach().contiguous()
    if len(w) != 13 or len(b) != 13 or len(li) != 5:
        raise RuntimeError('lpips_pack: needs 13 conv weights, 13 conv biases and 5 lin weights')
    with _guard_dev(dev):
        hw, hb, hl = _ptr_table(w, 'conv weight'), _ptr_table(b, 'conv bias'), _ptr_table(li, 'lin weight')
        rc = _lib.lib().occnerf_lpips_pack(hw, hb, hl, _chk(sh, torch.float32, 'shift'), _chk(sc, torch.float32, 'scale'),
                                           packed.data_ptr(), _stream(packed))
    _lib.check(rc, 'lpips_pack')
    return packed


def _lpips_layout(in0, in1):
    """(in0, in1, nhwc): NCHW-contiguous inputs as they are, NHWC-dense ones (a permuted [N,H,W,3] tensor) without a copy."""
    if in0.is_contiguous() and in1.is_contiguous():
        return in0, in1, 0
    p0, p1 = in0.permute(0, 2, 3, 1), in1.permute(0, 2, 3, 1)
    if p0.is_contiguous() and p1.is_contiguous():
        return in0, in1, 1
    return in0.contiguous(), in1.contiguous(), 0


def lpips_forward(packed, in0, in1, want_res=False):
    """val[N] (and res[5,N]) of LPIPS-VGG for in0, in1 [N,3,H,W]; returns (val, res, work, nhwc) -- the workspace carries the
    activations the backward needs."""
    if in0.dim() != 4 or in0.shape != in1.shape or in0.shape[1] != 3:
        raise RuntimeError(f'lpips: in0 and in1 must both be [N,3,H,W], got {tuple(in0.shape)} and {tuple(in1.shape)}')
    N, _, H, W = in0.shape
    in0, in1, nhwc = _lpips_layout(in0, in1)
    with _guard(in0):
        nw = int(_lib.lib().occnerf_lpips_workspace_floats(N, H, W))
        if nw < 0:
            raise RuntimeError(f'lpips: H and W must be >= 16 so that relu5_3 is not empty (got {H} x {W}), N >= 1')
        work = torch.empty(nw, device=in0.device, dtype=torch.float32)
        val = torch.empty(N, device=in0.device, dtype=torch.float32)
        res = torch.empty(5, N, device=in0.device, dtype=torch.float32) if want_res else None
        a0 = _chk(in0.permute(0, 2, 3, 1) if nhwc else in0, torch.float32, 'in0')
        a1 = _chk(in1.permute(0, 2, 3, 1) if nhwc else in1, torch.float32, 'in1')
        rc = _lib.lib().occnerf_lpips_forward(_chk(packed, torch.float32, 'packed'), a0, a1, N, H, W, nhwc, work.data_ptr(),
                                              val.data_ptr(), None if res is None else res.data_ptr(), _stream(in0))
    _lib.check(rc, 'lpips_forward')
    return val, res, work, nhwc


def lpips_backward(packed, work, shape, nhwc, gres, need0, need1):
    """d in0 / d in1 (None where not needed) from gres[5,N] = d loss / d res, on the workspace of the matching forward."""
    N, _, H, W = shape

    def alloc():
        return torch.empty((N, H, W, 3) if nhwc else (N, 3, H, W), device=work.device, dtype=torch.float32)
    d0 = alloc() if need0 else None
    d1 = alloc() if need1 else None
    with _guard(work):
        rc = _lib.lib().occnerf_lpips_backward(_chk(packed, torch.float32, 'packed'), _chk(work, torch.float32, 'work'), N,
                                               H, W, nhwc, _chk(gres, torch.float32, 'gres'),
                                               None if d0 is None else d0.data_ptr(), None if d1 is None else d1.data_ptr(),
                                               _stream(work))
    _lib.check(rc, 'lpips_backward')
    fix = (lambda t: None if t is None else t.permute(0, 3, 1, 2)) if nhwc else (lambda t: t)
    return fix(d0), fix(d1)


def patch_assemble(rgb, row_of_pix, n_patches, size, bgcolor01):
    """img[P,S,S,3] from the batch's rows (trainer.py:31-41 _unpack_imgs), background bgcolor01 where a pixel has no ray."""
    R = rgb.shape[0]
    img = torch.empty(n_patches, size, size, 3, device=rgb.device, dtype=torch.float32)
    bg, bgp = _host_f32(bgcolor01, 3)
    with _guard(rgb):
        rc = _lib.lib().occnerf_patch_assemble(_chk(rgb, torch.float32, 'rgb'), _chk(row_of_pix, torch.int32, 'row_of_pix'),
                                               R, int(n_patches), int(size), bgp, img.data_ptr(), _stream(rgb))
    _lib.check(rc, 'patch_assemble')
    return img


def patch_assemble_backward(d_img, pix_of_row):
    R = pix_of_row.shape[0]
    d_rgb = torch.empty(R, 3, device=d_img.device, dtype=torch.float32)
    with _guard(d_img):
        rc = _lib.lib().occnerf_patch_assemble_backward(_chk(d_img, torch.float32, 'd_img'),
                                                        _chk(pix_of_row, torch.int32, 'pix_of_row'), R, d_rgb.data_ptr(),
                                                        _stream(d_img))
    _lib.check(rc, 'patch_assemble_backward')
    return d_rgb


# ------------------------------------------------------------------ the training batch of a prepared dataset frame
PATCH_BATCH_KEYS = ('rays', 'near', 'far', 'target_rgbs', 'target_patches', 'patch_masks', 'patch_div_indices', 'xy_min',
                    'pix_of_row', 'row_of_pix', 'n_rows')


def alloc_patch_batch(n_patches, size, H, device):
    """The buffers occnerf_patch_batch fills, sized for R = n_patches * size^2 rows, plus its row-count scratch."""
    N, S = int(n_patches), int(size)
    rmax = N * S * S
    f32 = dict(device=device, dtype=torch.float32)
    i32 = dict(device=device, dtype=torch.int32)
    return {'rays': torch.zeros(2, rmax, 3, **f32), 'near': torch.zeros(rmax, 1, **f32), 'far': torch.zeros(rmax, 1, **f32),
            'target_rgbs': torch.zeros(rmax, 3, **f32), 'target_patches': torch.zeros(N, S, S, 3, **f32),
            'patch_masks': torch.zeros(N, S, S, device=device, dtype=torch.bool),
            'patch_div_indices': torch.zeros(N + 1, **i32), 'xy_min': torch.zeros(N, 2, **i32),
            'pix_of_row': torch.zeros(rmax, **i32), 'row_of_pix': torch.zeros(rmax, **i32), 'n_rows': torch.zeros(1, **i32),
            'row_counts': torch.zeros(2 * int(H), **i32)}


def patch_batch(image, alpha, rays8, box_mask, n_patches, size, u, subject_ratio, bgcolor, out=None):
    """The patch batch of one frame (include/occnerf_hip.h occnerf_patch_batch): image / alpha [H,W,3] uint8 on the device,
    rays8 / box_mask from gen_rays, u[n_patches,2] host uniforms in [0, 1), bgcolor[3] in 0..255 on the host.  -> the dict of
    alloc_patch_batch (filled in place when passed as `out`); the row count stays on the device in 'n_rows'."""
    return _patch_batch('occnerf_patch_batch', torch.uint8, image, alpha, rays8, box_mask, n_patches, size, u, subject_ratio,
                        bgcolor, out)


def patch_batch_f64(img64, alpha64, rays8, box_mask, n_patches, size, u, subject_ratio, bgcolor, out=None):
    """patch_batch on a frame resize_frame has written (include/occnerf_hip.h occnerf_patch_batch_f64): img64 / alpha64
    [H,W,3] float64 at the training size in the place of image / alpha; everything else as patch_batch."""
    return _patch_batch('occnerf_patch_batch_f64', torch.float64, img64, alpha64, rays8, box_mask, n_patches, size, u,
                        subject_ratio, bgcolor, out)


def _patch_batch(entry, dtype, image, alpha, rays8, box_mask, n_patches, size, u, subject_ratio, bgcolor, out):
    if not torch.is_tensor(image) or not torch.is_tensor(alpha) or image.dim() != 3 or alpha.dim() != 3:
        raise RuntimeError('patch_batch: image and alpha must be [H,W,3] tensors')
    H, W = int(image.shape[0]), int(image.shape[1])
    N, S = int(n_patches), int(size)
    if tuple(image.shape) != (H, W, 3) or tuple(alpha.shape) != (H, W, 3):
        raise RuntimeError(f'patch_batch: image and alpha must both be [H,W,3], got {tuple(image.shape)}, {tuple(alpha.shape)}')
    if rays8.numel() != H * W * 8 or box_mask.numel() != H * W:
        raise RuntimeError(f'patch_batch: rays8 / box_mask are not those of a {H} x {W} frame')
    if out is None:
        out = alloc_patch_batch(N, S, H, image.device)
    if out['target_patches'].shape != (N, S, S, 3) or out['row_counts'].numel() < 2 * H:
        raise RuntimeError('patch_batch: `out` was allocated for another patch count, patch size or image height')
    u0 = np.ascontiguousarray(np.asarray(u, dtype=np.float64).reshape(-1))
    if u0.size != 2 * N:
        raise RuntimeError(f'patch_batch: u must be [{N},2], got {np.asarray(u).shape}')
    bg, bgp = _host_f32(bgcolor, 3)
    floats = ('rays', 'near', 'far', 'target_rgbs', 'target_patches')
    ptr = {k: _chk(out[k], torch.bool if k == 'patch_masks' else torch.float32 if k in floats else torch.int32, k)
           for k in PATCH_BATCH_KEYS + ('row_counts',)}
    if any(out[k].device != image.device for k in ptr):
        raise RuntimeError('patch_batch: `out` is on another device than the frame')
    rmax = N * S * S
    want = {'rays': 6 * rmax, 'near': rmax, 'far': rmax, 'target_rgbs': 3 * rmax, 'target_patches': 3 * rmax,
            'patch_masks': rmax, 'patch_div_indices': N + 1, 'xy_min': 2 * N, 'pix_of_row': rmax, 'row_of_pix': rmax, 'n_rows': 1}
    for k, n in want.items():
        if out[k].numel() != n:
            raise RuntimeError(f'patch_batch: out[{k!r}] holds {out[k].numel()} elements, the batch needs {n}')
    with _guard(image):
        rc = getattr(_lib.lib(), entry)(
            _chk(image, dtype, 'image'), _chk(alpha, dtype, 'alpha'), _chk(rays8, torch.float32, 'rays8'),
            _chk(box_mask, torch.uint8, 'box_mask'), H, W, N, S, u0.ctypes.data_as(C.c_void_p), float(subject_ratio), bgp,
            ptr['row_counts'], ptr['rays'], ptr['near'], ptr['far'], ptr['target_rgbs'], ptr['target_patches'],
            ptr['patch_masks'], ptr['patch_div_indices'], ptr['xy_min'], ptr['pix_of_row'], ptr['row_of_pix'], ptr['n_rows'],
            _stream(image))
    _lib.check(rc, 'patch_batch')
    return out


# ------------------------------------------------------------------ a whole frame of a prepared dataset
WHOLE_FRAME_KEYS = ('ray_index', 'rays', 'near', 'far', 'target_rgbs', 'ray_alpha', 'truth_u8', 'gt_vis', 'gt_alpha')


def _whole_frame_shapes(H, W, R):
    return {'ray_index': ((R,), torch.int64), 'rays': ((2, R, 3), torch.float32), 'near': ((R, 1), torch.float32),
            'far': ((R, 1), torch.float32), 'target_rgbs': ((R, 3), torch.float32), 'ray_alpha': ((R, 3), torch.float64),
            'truth_u8': ((H, W, 3), torch.uint8), 'gt_vis': ((H, W), torch.float32), 'gt_alpha': ((H, W), torch.float32)}


def alloc_whole_frame(H, W, R, device):
    """The buffers occnerf_whole_frame_gather fills for a frame of R rays."""
    return {k: torch.empty(shape, device=device, dtype=dtype) for k, (shape, dtype) in _whole_frame_shapes(H, W, R).items()}


def whole_frame_count(box_mask, H, W, row_start=None):
    """row_start int32 [H+1] on the device: the box pixels above every image row, row_start[H] = the frame's ray count R
    (include/occnerf_hip.h occnerf_whole_frame_count).  Nothing is read back here."""
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or H * W >= 1 << 28:
        raise RuntimeError(f'whole_frame: H*W = {H} * {W} must be in [1, 2^28)')
    ptr = _chk(box_mask, torch.uint8, 'box_mask')
    if box_mask.numel() != H * W:
        raise RuntimeError(f'whole_frame: box_mask holds {box_mask.numel()} entries, a {H} x {W} frame has {H * W}')
    if row_start is None:
        row_start = torch.empty(H + 1, device=box_mask.device, dtype=torch.int32)
    rs = _chk(row_start, torch.int32, 'row_start')
    if row_start.numel() != H + 1 or row_start.device != box_mask.device:
        raise RuntimeError(f'whole_frame: row_start must be int32 [{H + 1}] on the device of box_mask')
    with _guard(box_mask):
        rc = _lib.lib().occnerf_whole_frame_count(ptr, H, W, rs, _stream(box_mask))
    _lib.check(rc, 'whole_frame_count')
    return row_start


def _frame_rows(who, H, W, rays8, box_mask, row_start, R, image=None, alpha=None):
    """What whole_frame and view_frame check alike, under the caller's name, once the caller has refused an H*W out of
    range in its own words: rays8 / box_mask (and whole_frame's image / alpha) as those of one H x W frame on one device,
    then row_start and R -- given together, or both None: counted here and read back with one blocking copy.
    -> (row_start, R, the pointers of (rays8, box_mask, row_start))."""
    pr, pb = _chk(rays8, torch.float32, 'rays8'), _chk(box_mask, torch.uint8, 'box_mask')
    if rays8.numel() != H * W * 8 or box_mask.numel() != H * W:
        raise RuntimeError(f'{who}: rays8 / box_mask are not those of a {H} x {W} frame')
    if any(t is not None and t.device != rays8.device for t in (image, alpha, box_mask)):
        raise RuntimeError(f"{who}: {'rays8' if image is None else 'image, alpha, rays8'} and box_mask must be on one device")
    if (row_start is None) != (R is None):
        raise RuntimeError(f'{who}: row_start and R come together (whole_frame_count and its row_start[H])')
    if row_start is None:
        row_start = whole_frame_count(box_mask, H, W)
        R = int(row_start[H].item())
    R = int(R)
    ps = _chk(row_start, torch.int32, 'row_start')
    if row_start.numel() != H + 1 or row_start.device != rays8.device:
        raise RuntimeError(f'{who}: row_start must be int32 [{H + 1}] on the frame\'s device')
    if R < 0 or R > H * W:
        raise RuntimeError(f'{who}: R = {R} is outside [0, {H * W}]')
    return row_start, R, (pr, pb, ps)


def whole_frame(image, alpha, rays8, box_mask, bgcolor, row_start=None, R=None, out=None):
    """One frame of a prepared dataset as PreparedDataset.whole_frame() builds it on the host, plus the per-pixel maps of the
    metrics (include/occnerf_hip.h occnerf_whole_frame_gather): image / alpha [H,W,3] uint8 on the device, rays8 / box_mask
    from gen_rays, bgcolor[3] in 0..255 on the host.  -> dict of WHOLE_FRAME_KEYS.
    row_start, R: the result of whole_frame_count and the host copy of row_start[H] (the loader reads it from pinned memory
    behind an event); both None: counted here and read back with one blocking copy.  out: a dict of alloc_whole_frame(H, W, R)
    to fill in place."""
    return _whole_frame('occnerf_whole_frame_gather', torch.uint8, image, alpha, rays8, box_mask, bgcolor, row_start, R, out)


def whole_frame_f64(img64, alpha64, rays8, box_mask, bgcolor, row_start=None, R=None, out=None):
    """whole_frame on a frame resize_frame has written (include/occnerf_hip.h occnerf_whole_frame_gather_f64): img64 /
    alpha64 [H,W,3] float64 at the training size in the place of image / alpha; bgcolor still colours truth_u8 outside the
    box.  Everything else as whole_frame."""
    return _whole_frame('occnerf_whole_frame_gather_f64', torch.float64, img64, alpha64, rays8, box_mask, bgcolor, row_start, R,
                        out)


def _whole_frame(entry, dtype, image, alpha, rays8, box_mask, bgcolor, row_start, R, out):
    if not torch.is_tensor(image) or not torch.is_tensor(alpha) or image.dim() != 3 or alpha.dim() != 3:
        raise RuntimeError('whole_frame: image and alpha must be [H,W,3] tensors')
    H, W = int(image.shape[0]), int(image.shape[1])
    if tuple(image.shape) != (H, W, 3) or tuple(alpha.shape) != (H, W, 3):
        raise RuntimeError(f'whole_frame: image and alpha must both be [H,W,3], got {tuple(image.shape)}, {tuple(alpha.shape)}')
    if H * W >= 1 << 28:
        raise RuntimeError(f'whole_frame: H*W = {H} * {W} must be below 2^28')
    pi, pa = _chk(image, dtype, 'image'), _chk(alpha, dtype, 'alpha')
    row_start, R, (pr, pb, ps) = _frame_rows('whole_frame', H, W, rays8, box_mask, row_start, R, image, alpha)
    if out is None:
        out = alloc_whole_frame(H, W, R, image.device)
    ptr = {}
    for k, (shape, dtype) in _whole_frame_shapes(H, W, R).items():
        if k not in out or not torch.is_tensor(out[k]) or tuple(out[k].shape) != shape:
            got = tuple(out[k].shape) if k in out and torch.is_tensor(out[k]) else None
            raise RuntimeError(f'whole_frame: out[{k!r}] must be {shape} for R = {R}, got {got}')
        ptr[k] = _chk(out[k], dtype, k)
        if out[k].device != image.device:
            raise RuntimeError('whole_frame: `out` is on another device than the frame')
    bg, bgp = _host_f32(bgcolor, 3)
    with _guard(image):
        rc = getattr(_lib.lib(), entry)(
            pi, pa, pr, pb, H, W, bgp, ps, R, ptr['ray_index'], ptr['rays'], ptr['near'], ptr['far'], ptr['target_rgbs'],
            ptr['ray_alpha'], ptr['truth_u8'], ptr['gt_vis'], ptr['gt_alpha'], _stream(image))
    _lib.check(rc, 'whole_frame_gather')
    return out


# ------------------------------------------------------------------ the rays of a camera without a photograph
def view_frame(rays8, box_mask, H, W, row_start=None, R=None):
    """The rays of a novel view (include/occnerf_hip.h occnerf_view_frame_gather): rays8 / box_mask from gen_rays for an
    H x W camera -> {'ray_index' int64 [R], 'rays' [2,R,3], 'near' [R,1], 'far' [R,1]}, the box hits in np.nonzero order.
    No image is read and no per-pixel map written.  row_start, R: as for whole_frame (whole_frame_count's result and the host
    copy of row_start[H]); both None: counted here and read back with one blocking copy."""
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or H * W >= 1 << 28:
        raise RuntimeError(f'view_frame: H*W = {H} * {W} must be in [1, 2^28)')
    row_start, R, (pr, pb, ps) = _frame_rows('view_frame', H, W, rays8, box_mask, row_start, R)
    dev = rays8.device
    out = {'ray_index': torch.empty(R, device=dev, dtype=torch.int64), 'rays': torch.empty(2, R, 3, device=dev),
           'near': torch.empty(R, 1, device=dev), 'far': torch.empty(R, 1, device=dev)}
    with _guard(rays8):
        rc = _lib.lib().occnerf_view_frame_gather(pr, pb, H, W, ps, R, out['ray_index'].data_ptr(), out['rays'].data_ptr(),
                                                  out['near'].data_ptr(), out['far'].data_ptr(), _stream(rays8))
    _lib.check(rc, 'view_frame_gather')
    return out


# ------------------------------------------------------------------ undistorting a frame at open
def undistort_u8(image, mask, K, D, window=None, out=None):
    """occnerf_amd.undistort.undistort_u8 on the device (include/occnerf_hip.h occnerf_undistort_u8): image [H,W,3] uint8 and
    mask [H,W,3] uint8 or None on one device, K the 3x3 camera matrix as stored and D 4 / 5 / 8 coefficients on the host,
    window (y0, x0, h, w) or None for the whole image -> (image', mask' or None), uint8 [h,w,3], on the current stream.
    out: the pair to fill in place (the second entry None without a mask); it must not share memory with the inputs."""
    from . import undistort as und
    if not torch.is_tensor(image) or image.dim() != 3 or image.shape[2] != 3:
        raise RuntimeError('undistort_u8: image must be a [H,W,3] tensor')
    H, W = int(image.shape[0]), int(image.shape[1])
    if H * W >= 1 << 28:
        raise RuntimeError(f'undistort_u8: H*W = {H} * {W} must be below 2^28')
    pi, pm = _chk(image, torch.uint8, 'image'), _opt(mask, torch.uint8, 'mask')
    if mask is not None and (tuple(mask.shape) != (H, W, 3) or mask.device != image.device):
        raise RuntimeError(f'undistort_u8: mask must be [{H},{W},3] on the device of image')
    k, d = und.camera(K).reshape(9), und.coefficients(D)
    y0, x0, h, w = und.check_window(window, H, W)
    if out is None:
        out = (torch.empty(h, w, 3, device=image.device, dtype=torch.uint8),
               None if mask is None else torch.empty(h, w, 3, device=image.device, dtype=torch.uint8))
    oi, om = out
    if (om is None) != (mask is None):
        raise RuntimeError('undistort_u8: out holds a mask exactly when a mask is given')
    po, pom = _chk(oi, torch.uint8, 'out image'), _opt(om, torch.uint8, 'out mask')
    if any(t is not None and (tuple(t.shape) != (h, w, 3) or t.device != image.device) for t in (oi, om)):
        raise RuntimeError(f'undistort_u8: out must be [{h},{w},3] on the device of image')
    with _guard(image):
        rc = _lib.lib().occnerf_undistort_u8(pi, pm, H, W, k.ctypes.data, d.ctypes.data, y0, x0, h, w, po, pom, _stream(image))
    _lib.check(rc, 'undistort_u8')
    return oi, om


# ------------------------------------------------------------------ resizing a prepared frame to the training size
_RESIZE_TABLES = ('x_lanczos', 'y_lanczos', 'x_bilinear', 'y_bilinear')


def upload_resize_tables(tables, device):
    """resize.frame_tables(H, W, s) -> what resize_frame takes: the four tables on `device` beside their host copies (the
    entry checks the host offsets before it launches).  Built once per dataset."""
    if torch.device(device).type != 'cuda':
        raise RuntimeError(f'upload_resize_tables: {device} is not a GPU; resize.resize_blend is the host path')
    out = {'size': tuple(int(v) for v in tables['size']), 'src_size': tuple(int(v) for v in tables['src_size']), 'device': {}}
    for k in _RESIZE_TABLES:
        off, wgt = tables[k]
        off, wgt = np.ascontiguousarray(off, dtype=np.int32), np.ascontiguousarray(wgt, dtype=np.float32)
        n, taps = out['size'][0 if k[0] == 'y' else 1], 8 if k.endswith('lanczos') else 2
        if off.shape != (n, taps) or wgt.shape != (n, taps):
            raise RuntimeError(f'upload_resize_tables: {k} must be [{n},{taps}], got offsets {off.shape}, weights {wgt.shape}')
        out[k] = (off, wgt)
        out['device'][k] = (torch.from_numpy(off).to(device), torch.from_numpy(wgt).to(device))
    return out


def alloc_resize_frame(h, w, device):
    """(img64, alpha64): the float64 frame resize_frame fills, 48 bytes per training pixel."""
    return (torch.empty(int(h), int(w), 3, device=device, dtype=torch.float64),
            torch.empty(int(h), int(w), 3, device=device, dtype=torch.float64))


def resize_frame(image, mask, tables, bgcolor=None, out=None):
    """occnerf_amd.resize.resize_blend on the device (include/occnerf_hip.h occnerf_resize_frame): image [H,W,3] uint8 or
    None (the mask alone) and mask [H,W,3] uint8 on one device, tables from upload_resize_tables for that device and size,
    bgcolor[3] in 0..255 on the host -> (img64 or None, alpha64), float64 [h,w,3], on the current stream.  out: the pair to
    fill in place (the first entry None without an image); it must not share memory with the inputs."""
    if not torch.is_tensor(mask) or mask.dim() != 3 or mask.shape[2] != 3:
        raise RuntimeError('resize_frame: mask must be a [H,W,3] tensor')
    H, W = int(mask.shape[0]), int(mask.shape[1])
    if H * W >= 1 << 28:
        raise RuntimeError(f'resize_frame: H*W = {H} * {W} must be below 2^28')
    pm, pi = _chk(mask, torch.uint8, 'mask'), _opt(image, torch.uint8, 'image')
    if image is not None and (tuple(image.shape) != (H, W, 3) or image.device != mask.device):
        raise RuntimeError(f'resize_frame: image must be [{H},{W},3] on the device of mask')
    if not isinstance(tables, dict) or 'device' not in tables:
        raise RuntimeError('resize_frame: tables must come from upload_resize_tables')
    if tuple(tables['src_size']) != (H, W):
        raise RuntimeError(f"resize_frame: the tables are those of a {tables['src_size'][1]} x {tables['src_size'][0]} frame, "
                           f'the mask is {W} x {H}')
    h, w = tables['size']
    if image is not None and bgcolor is None:
        raise RuntimeError('resize_frame: an image is blended over bgcolor, which is None')
    if out is None:
        pair = alloc_resize_frame(h, w, mask.device)
        out = (None if image is None else pair[0], pair[1])
    oi, oa = out
    if (oi is None) != (image is None):
        raise RuntimeError('resize_frame: out holds an image exactly when an image is given')
    po, pa = _opt(oi, torch.float64, 'out image'), _chk(oa, torch.float64, 'out alpha')
    if any(t is not None and (tuple(t.shape) != (h, w, 3) or t.device != mask.device) for t in (oi, oa)):
        raise RuntimeError(f'resize_frame: out must be [{h},{w},3] on the device of mask')
    dev, host = [], []
    for k in _RESIZE_TABLES:
        off, wgt = tables['device'][k]
        if off.device != mask.device:
            raise RuntimeError('resize_frame: the tables are on another device than the frame')
        dev += [_chk(off, torch.int32, k + ' offsets'), _chk(wgt, torch.float32, k + ' weights')]
        host.append(tables[k][0].ctypes.data_as(C.c_void_p))
    bgp = None if image is None else _host_f32(bgcolor, 3)
    with _guard(mask):
        rc = _lib.lib().occnerf_resize_frame(pi, pm, H, W, h, w, *dev, *host, None if bgp is None else bgp[1], po, pa,
                                             _stream(mask))
    _lib.check(rc, 'resize_frame')
    return oi, oa


# ------------------------------------------------------------------ the body as a triangle mesh
def _mesh_field(who, field):
    if not torch.is_tensor(field) or field.dim() != 3:
        raise RuntimeError(f'{who}: field must be a [nz,ny,nx] tensor')
    ptr = _chk(field, torch.float32, 'field')
    nz, ny, nx = (int(s) for s in field.shape)
    if min(nx, ny, nz) < 2 or nx * ny * nz >= 1 << 31:
        raise RuntimeError(f'{who}: a {nx} x {ny} x {nz} grid: every axis needs 2 points, all of them fewer than 2^31')
    return ptr, nx, ny, nz


def _mesh_points(name, x):
    """The address of x, float32 [V,3] points on the GPU; `name`: the entry and the argument, for the refusal."""
    ptr = _chk(x, torch.float32, name)
    if x.dim() != 2 or x.shape[1] != 3:
        raise RuntimeError(f'{name} must be float32 [V,3], got {tuple(x.shape)}')
    return ptr


def _mesh_bgcolor(bgcolor):
    """bgcolor, 3 values 0..255 on the host, as the uint8 [3] the resolves take: rounded to nearest, clamped."""
    return np.ascontiguousarray(np.clip(np.rint(np.asarray(bgcolor, dtype=np.float64).reshape(3)), 0, 255).astype(np.uint8))


def mesh_count(field, level):
    """Triangles of every row of cubes (z, y) of field [nz,ny,nx] float32 at the iso level (compared in float32; include/
    occnerf_hip.h occnerf_mesh_count) -> int32 [(nz-1)*(ny-1)] on the device.  Nothing is read back here."""
    ptr, nx, ny, nz = _mesh_field('mesh_count', field)
    row_count = torch.empty((nz - 1) * (ny - 1), device=field.device, dtype=torch.int32)
    with _guard(field):
        rc = _lib.lib().occnerf_mesh_count(ptr, nx, ny, nz, float(np.float32(level)), row_count.data_ptr(), _stream(field))
    _lib.check(rc, 'mesh_count')
    return row_count


def mesh_emit(field, level, row_start, T, out=None):
    """The vertex keys of the T triangles (occnerf_mesh_emit): row_start int64 [(nz-1)*(ny-1)], the exclusive prefix of
    mesh_count's result, T its total on the host -> tri_keys int64 [T,3] in the order (z, y, x, tetrahedron, triangle).
    out: an int64 buffer of at least T rows of 3 to fill in place; rows at and past T are not written."""
    ptr, nx, ny, nz = _mesh_field('mesh_emit', field)
    T = int(T)
    if T < 0:
        raise RuntimeError(f'mesh_emit: T = {T} is negative')
    ps = _chk(row_start, torch.int64, 'row_start')
    if row_start.numel() != (nz - 1) * (ny - 1) or row_start.device != field.device:
        raise RuntimeError(f'mesh_emit: row_start must be int64 [{(nz - 1) * (ny - 1)}] on the device of field')
    if out is None:
        out = torch.empty(T, 3, device=field.device, dtype=torch.int64)
    po = _chk(out, torch.int64, 'tri_keys')
    if out.numel() < 3 * T or out.device != field.device:
        raise RuntimeError(f'mesh_emit: tri_keys must hold {T} rows of 3 on the device of field')
    with _guard(field):
        rc = _lib.lib().occnerf_mesh_emit(ptr, nx, ny, nz, float(np.float32(level)), ps, T, po if T else None, _stream(field))
    _lib.check(rc, 'mesh_emit')
    return out


def mesh_vertices(keys, field, level, bbox_min, h):
    """float32 [V,3] positions of the welded vertex keys (int64 [V], occnerf_mesh_vertices): the level's crossing on each
    key's edge in fp64; bbox_min[3] and the voxel edge h on the host."""
    ptr, nx, ny, nz = _mesh_field('mesh_vertices', field)
    pk = _chk(keys, torch.int64, 'keys')
    if keys.dim() != 1 or keys.device != field.device:
        raise RuntimeError('mesh_vertices: keys must be int64 [V] on the device of field')
    V = int(keys.numel())
    pos = torch.empty(V, 3, device=field.device, dtype=torch.float32)
    bmin = np.ascontiguousarray(np.asarray(bbox_min, dtype=np.float64).reshape(3))
    with _guard(field):
        rc = _lib.lib().occnerf_mesh_vertices(pk if V else None, V, ptr, nx, ny, nz, float(np.float32(level)),
                                              bmin.ctypes.data_as(C.c_void_p), float(h), pos.data_ptr() if V else None,
                                              _stream(field))
    _lib.check(rc, 'mesh_vertices')
    return pos


# ------------------------------------------------------------------ connected components of the mesh
MESH_LABEL_MAX_PASSES = 256
MESH_RECORD_COLUMNS = ('label', 'vertices', 'triangles', 'boundary_vertices', 'smin', 'smax', 'volume6_q')


def _mesh_faces(who, faces, V, dev):
    pf = _chk(faces, torch.int32, f'{who}: faces')
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.device != dev:
        raise RuntimeError(f'{who}: faces must be int32 [T,3] on the device of the vertices, got {tuple(faces.shape)}')
    T = int(faces.shape[0])
    if T >= 1 << 31 or V >= 1 << 31:
        raise RuntimeError(f'{who}: T = {T} / V = {V} reach the limit of 2^31')
    return pf, T


def mesh_label(faces, V, max_passes=MESH_LABEL_MAX_PASSES):
    """(labels int32 [V] on the device of faces, passes): labels[v] = the smallest vertex index of v's component of the mesh
    faces int32 [T,3] over V vertices (occnerf_mesh_label_pass, repeated until a pass changes nothing; one blocking read of
    two words per pass).  A face that names a vertex outside [0, V) and max_passes passes without a fixed point raise; partial
    labels are never returned."""
    if not torch.is_tensor(faces):
        raise RuntimeError('mesh_label: faces must be a tensor')
    V, max_passes = int(V), int(max_passes)
    if V < 0 or max_passes < 1:
        raise RuntimeError(f'mesh_label: V = {V} must be >= 0 and max_passes = {max_passes} >= 1')
    pf, T = _mesh_faces('mesh_label', faces, V, faces.device)
    labels = torch.arange(V, device=faces.device, dtype=torch.int32)
    if V == 0:
        if T:
            raise RuntimeError(f'mesh_label: {T} faces over no vertex')
        return labels, 0
    status = torch.zeros(2, device=faces.device, dtype=torch.int32)
    for passes in range(1, max_passes + 1):
        status.zero_()
        with _guard(faces):
            rc = _lib.lib().occnerf_mesh_label_pass(pf if T else None, T, V, labels.data_ptr(), status.data_ptr(), _stream(faces))
        _lib.check(rc, 'mesh_label_pass')
        changed, bad = status.tolist()
        if bad:
            raise RuntimeError(f'mesh_label: a face names a vertex outside [0, {V})')
        if not changed:
            return labels, passes
    raise RuntimeError(f'mesh_label: no pass left the labels unchanged within max_passes = {max_passes} ({T} triangles, {V} vertices)')


def mesh_component_ranks(labels):
    """(vrank int32 [V], roots int32 [C]): the rank of every vertex's component among the components in ascending label order,
    and the labels in that order.  Plumbing (torch.cumsum) between the launches; C is read back with one blocking copy."""
    V = int(labels.numel())
    is_root = labels == torch.arange(V, device=labels.device, dtype=torch.int32)
    rank = (torch.cumsum(is_root, 0, dtype=torch.int32) - 1)
    return rank[labels.long()].contiguous(), torch.nonzero(is_root).reshape(-1).to(torch.int32)


def mesh_component_stats(verts, faces, vrank, n_comp, bbox_min, h, shape):
    """The records of the n_comp = C components (occnerf_mesh_component_stats; include/occnerf_hip.h): verts float32 [V,3], faces int32
    [T,3], vrank int32 [V] (mesh_component_ranks), bbox_min[3] / h on the host, shape = (nx, ny, nz) of the grid -> (counts
    int32 [C,3]: vertices, triangles, boundary vertices; box int32 [C,6]: smin, smax; vol6 int64 [C]) on the device."""
    pv = _mesh_points('mesh_component_stats: verts', verts)
    V, dev, n_comp = int(verts.shape[0]), verts.device, int(n_comp)
    pf, T = _mesh_faces('mesh_component_stats', faces, V, dev)
    pr = _chk(vrank, torch.int32, 'mesh_component_stats: vrank')
    if tuple(vrank.shape) != (V,) or vrank.device != dev:
        raise RuntimeError(f'mesh_component_stats: vrank must be int32 [{V}] on the device of verts')
    nx, ny, nz = (int(s) for s in shape)
    h = float(h)
    if not (0.0 < h < float('inf')) or min(nx, ny, nz) < 2 or max(nx, ny, nz) > 1 << 20 or not 0 <= n_comp <= V:
        raise RuntimeError(f'mesh_component_stats: h = {h} must be positive and finite, every axis of the {nx} x {ny} x {nz} grid '
                           f'2 .. 2^20 points, C = {n_comp} within [0, V = {V}]')
    counts = torch.zeros(n_comp, 3, device=dev, dtype=torch.int32)
    box = torch.empty(n_comp, 6, device=dev, dtype=torch.int32)
    box[:, :3], box[:, 3:] = torch.iinfo(torch.int32).max, torch.iinfo(torch.int32).min
    vol6 = torch.zeros(n_comp, device=dev, dtype=torch.int64)
    if V == 0 or n_comp == 0:
        return counts, box, vol6
    bmin = np.ascontiguousarray(np.asarray(bbox_min, dtype=np.float64).reshape(3))
    with _guard(verts):
        rc = _lib.lib().occnerf_mesh_component_stats(pv, V, pf if T else None, T, pr, n_comp, bmin.ctypes.data_as(C.c_void_p), h, nx, ny,
                                                     nz, counts.data_ptr(), box.data_ptr(), vol6.data_ptr(), _stream(verts))
    _lib.check(rc, 'mesh_component_stats')
    return counts, box, vol6


def mesh_components(verts, faces, bbox_min, h, shape, max_passes=MESH_LABEL_MAX_PASSES):
    """(labels int32 [V], records) of the mesh verts float32 [V,3] / faces int32 [T,3]: labels[v] = the
    smallest vertex index connected to v through faces; records: a dict of device tensors, one row per component in ascending
    label order -- label, vertices, triangles, boundary_vertices int32 [C], smin, smax int32 [C,3] (the box in 1/1024 voxel
    from bbox_min), volume6_q int64 [C] -- and 'passes', the labelling passes taken (an int)."""
    if not torch.is_tensor(verts) or verts.dim() != 2 or verts.shape[1] != 3:
        raise RuntimeError('mesh_components: verts must be a float32 [V,3] tensor')
    _chk(verts, torch.float32, 'mesh_components: verts')
    if not torch.is_tensor(faces) or faces.device != verts.device:
        raise RuntimeError('mesh_components: faces must be a tensor on the device of verts')
    labels, passes = mesh_label(faces, int(verts.shape[0]), max_passes)
    vrank, roots = mesh_component_ranks(labels)
    counts, box, vol6 = mesh_component_stats(verts, faces, vrank, int(roots.numel()), bbox_min, h, shape)
    return labels, {'label': roots, 'vertices': counts[:, 0].contiguous(), 'triangles': counts[:, 1].contiguous(),
                    'boundary_vertices': counts[:, 2].contiguous(), 'smin': box[:, :3].contiguous(),
                    'smax': box[:, 3:].contiguous(), 'volume6_q': vol6, 'passes': passes}


def mesh_pose(x_c, Rs, Ts, vol, bbox_min, bbox_scale, candidates=3, max_iter=20, tol=1e-7):
    """Observation-space positions of canonical points (occnerf_mesh_pose): x_c float32 [V,3], Rs [nb,3,3],
    Ts [nb,3] and vol [>= nb,G,G,G] (only the first nb channels are read: the background channel is dropped) as
    Network.render_preamble returns them, bbox_min[3] / bbox_scale[3] on the host -> (p float32 [V,3], flag uint8 [V],
    iters uint8 [V], resid float32 [V]) on the device of x_c.  V = 0 launches nothing."""
    px = _mesh_points('mesh_pose: x_c', x_c)
    pR, pT, pv = _chk(Rs, torch.float32, 'mesh_pose: Rs'), _chk(Ts, torch.float32, 'mesh_pose: Ts'), _chk(vol, torch.float32, 'mesh_pose: vol')
    nb = int(Rs.shape[0]) if Rs.dim() == 3 else -1
    if nb < 1 or tuple(Rs.shape) != (nb, 3, 3) or tuple(Ts.shape) != (nb, 3):
        raise RuntimeError(f'mesh_pose: Rs must be [nb,3,3] and Ts [nb,3], got {tuple(Rs.shape)} and {tuple(Ts.shape)}')
    if vol.dim() != 4 or vol.shape[0] < nb or not (vol.shape[1] == vol.shape[2] == vol.shape[3]):
        raise RuntimeError(f'mesh_pose: vol must be [>= {nb},G,G,G], got {tuple(vol.shape)}')
    if not (Rs.device == Ts.device == vol.device == x_c.device):
        raise RuntimeError('mesh_pose: x_c, Rs, Ts and vol must be on one device')
    candidates, max_iter, tol = int(candidates), int(max_iter), float(tol)
    if not 1 <= candidates <= 8:
        raise RuntimeError(f'mesh_pose: candidates = {candidates} outside 1..8')
    if not 1 <= max_iter <= 255:
        raise RuntimeError(f'mesh_pose: max_iter = {max_iter} outside 1..255')
    if not (0.0 <= tol < float('inf')):
        raise RuntimeError(f'mesh_pose: tol = {tol} must be a finite number >= 0')
    V, dev = int(x_c.shape[0]), x_c.device
    p = torch.empty(V, 3, device=dev, dtype=torch.float32)
    flag = torch.empty(V, device=dev, dtype=torch.uint8)
    iters = torch.empty(V, device=dev, dtype=torch.uint8)
    resid = torch.empty(V, device=dev, dtype=torch.float32)
    if V == 0:
        return p, flag, iters, resid
    _kmin, pmin = _host_f32(bbox_min, 3)
    _ksc, psc = _host_f32(bbox_scale, 3)
    with _guard(x_c):
        rc = _lib.lib().occnerf_mesh_pose(px, V, pR, pT, pv, nb, int(vol.shape[-1]), pmin, psc, candidates, max_iter, tol,
                                          p.data_ptr(), flag.data_ptr(), iters.data_ptr(), resid.data_ptr(), _stream(x_c))
    _lib.check(rc, 'mesh_pose')
    return p, flag, iters, resid


# ------------------------------------------------------------------ the mesh as a rig
def mesh_skin(x_c, vol, bbox_min, bbox_scale, K=4):
    """The K (4 or 8) skinning influences of canonical points (occnerf_mesh_skin): x_c float32 [V,3], vol [nb,G,G,G]: what
    Network.render_preamble returns with the background channel dropped (vol[:nb], as mesh_pose reads it), bbox_min[3] / bbox_scale[3] on the host ->
    (joints uint8 [V,K], weights float32 [V,K], count uint8 [V], kept float32 [V]) on the device of x_c.  V = 0 launches
    nothing."""
    px = _mesh_points('mesh_skin: x_c', x_c)
    pv = _chk(vol, torch.float32, 'mesh_skin: vol')
    K = int(K)
    if K not in (4, 8):
        raise RuntimeError(f'mesh_skin: K = {K} is neither 4 nor 8')
    if vol.dim() != 4 or not (vol.shape[1] == vol.shape[2] == vol.shape[3]) or vol.device != x_c.device:
        raise RuntimeError(f'mesh_skin: vol must be [nb,G,G,G] on the device of x_c, got {tuple(vol.shape)}')
    nb = int(vol.shape[0])
    if not 1 <= nb <= 32:
        raise RuntimeError(f'mesh_skin: nb = {nb} outside 1..32 (drop the background channel: vol[:nb])')
    V, dev = int(x_c.shape[0]), x_c.device
    joints = torch.empty(V, K, device=dev, dtype=torch.uint8)
    weights = torch.empty(V, K, device=dev, dtype=torch.float32)
    count = torch.empty(V, device=dev, dtype=torch.uint8)
    kept = torch.empty(V, device=dev, dtype=torch.float32)
    if V == 0:
        return joints, weights, count, kept
    _kmin, pmin = _host_f32(bbox_min, 3)
    _ksc, psc = _host_f32(bbox_scale, 3)
    with _guard(x_c):
        rc = _lib.lib().occnerf_mesh_skin(px, V, pv, nb, int(vol.shape[-1]), pmin, psc, K, joints.data_ptr(), weights.data_ptr(),
                                          count.data_ptr(), kept.data_ptr(), _stream(x_c))
    _lib.check(rc, 'mesh_skin')
    return joints, weights, count, kept


def mesh_lbs(x_c, joints, weights, Rs, Ts, target=None, target_flag=None, max_delta=0.05, joints_checked=False):
    """Forward linear blend skinning of the rig for F frames at once (occnerf_mesh_lbs): x_c float32 [V,3], mesh_skin's joints
    uint8 [V,K] / weights float32 [V,K], the frames' backward bases Rs [F,nb,3,3] / Ts [F,nb,3] -> posed float32 [F,V,3]; with
    target float32 [F,V,3] and target_flag uint8 [F,V] -> (posed, delta float32 [F,V,3], dflag uint8 [F,V]): the displacement
    of the canonical vertex that makes its skinned position the target, 0 and flagged where it is not to be had or exceeds
    max_delta.  A joint index >= nb is refused by name before anything is launched (one blocking read of the joints' maximum;
    joints_checked=True: the caller has made that test).  V = 0 launches nothing."""
    px = _mesh_points('mesh_lbs: x_c', x_c)
    V, dev = int(x_c.shape[0]), x_c.device
    pj, pw = _chk(joints, torch.uint8, 'mesh_lbs: joints'), _chk(weights, torch.float32, 'mesh_lbs: weights')
    K = int(joints.shape[1]) if joints.dim() == 2 else -1
    if K not in (4, 8) or tuple(joints.shape) != (V, K) or tuple(weights.shape) != (V, K):
        raise RuntimeError(f'mesh_lbs: joints and weights must be [{V},K] with K 4 or 8, got {tuple(joints.shape)} and '
                           f'{tuple(weights.shape)}')
    pR, pT = _chk(Rs, torch.float32, 'mesh_lbs: Rs'), _chk(Ts, torch.float32, 'mesh_lbs: Ts')
    F, nb = (int(Rs.shape[0]), int(Rs.shape[1])) if Rs.dim() == 4 else (-1, -1)
    if F < 1 or nb < 1 or tuple(Rs.shape) != (F, nb, 3, 3) or tuple(Ts.shape) != (F, nb, 3):
        raise RuntimeError(f'mesh_lbs: Rs must be [F,nb,3,3] and Ts [F,nb,3] with F >= 1, got {tuple(Rs.shape)} and {tuple(Ts.shape)}')
    if not 1 <= nb <= 32 or F > 65535:
        raise RuntimeError(f'mesh_lbs: nb = {nb} outside 1..32 or F = {F} above 65535')
    max_delta = float(max_delta)
    if not (0.0 <= max_delta < float('inf')):
        raise RuntimeError(f'mesh_lbs: max_delta = {max_delta} must be a finite number >= 0')
    if (target is None) != (target_flag is None):
        raise RuntimeError('mesh_lbs: target and target_flag come together')
    pt = pf = None
    if target is not None:
        pt, pf = _chk(target, torch.float32, 'mesh_lbs: target'), _chk(target_flag, torch.uint8, 'mesh_lbs: target_flag')
        if tuple(target.shape) != (F, V, 3) or tuple(target_flag.shape) != (F, V):
            raise RuntimeError(f'mesh_lbs: target must be [{F},{V},3] and target_flag [{F},{V}], got {tuple(target.shape)} and '
                               f'{tuple(target_flag.shape)}')
    if not all(t.device == dev for t in (joints, weights, Rs, Ts) + (() if target is None else (target, target_flag))):
        raise RuntimeError('mesh_lbs: every tensor must be on the device of x_c')
    if V and not joints_checked:
        hi = int(joints.max().item())
        if hi >= nb:
            raise RuntimeError(f'mesh_lbs: joint index {hi} outside [0, {nb})')
    posed = torch.empty(F, V, 3, device=dev, dtype=torch.float32)
    delta = dflag = None
    if target is not None:
        delta = torch.empty(F, V, 3, device=dev, dtype=torch.float32)
        dflag = torch.empty(F, V, device=dev, dtype=torch.uint8)
    if V:
        with _guard(x_c):
            rc = _lib.lib().occnerf_mesh_lbs(px, V, pj, pw, K, pR, pT, F, nb, pt, pf, max_delta, posed.data_ptr(),
                                             None if delta is None else delta.data_ptr(),
                                             None if dflag is None else dflag.data_ptr(), _stream(x_c))
        _lib.check(rc, 'mesh_lbs')
    return posed if target is None else (posed, delta, dflag)


# ------------------------------------------------------------------ the mesh seen through a camera
MESH_RASTER_COUNTS = ('index', 'near', 'guard', 'area', 'offscreen', 'wide', 'covered')
MESH_RASTER_MAX_SIDE, MESH_RASTER_MAX_PIXELS = 16384, 1 << 28


def _host_matrix64(vals, shape, name):
    a = np.ascontiguousarray(np.asarray(vals.detach().cpu().numpy() if torch.is_tensor(vals) else vals, dtype=np.float64))
    if a.shape != shape:
        raise RuntimeError(f'{name} must be {shape[0]}x{shape[1]}, got {a.shape}')
    return a


def mesh_project(pos, K, E):
    """Vertices through a pinhole camera (occnerf_mesh_project): pos float32 [V,3] on the device, K 3x3 and E 4x4 on the host
    (float64; E is the camera seen from the space of pos) -> (xy int32 [V,2] in 1/256 pixel, z float64 [V], vflag uint8 [V]: 1
    nearer than a millimetre, 2 past the guard band).  V = 0 launches nothing."""
    pp = _mesh_points('mesh_project: pos', pos)
    K, E = _host_matrix64(K, (3, 3), 'mesh_project: K'), _host_matrix64(E, (4, 4), 'mesh_project: E')
    if K[0, 1] != 0.0:
        raise NotImplementedError(f'mesh_project: skew K[0,1] = {K[0, 1]!r} is not built')
    V, dev = int(pos.shape[0]), pos.device
    if V >= 1 << 31:
        raise RuntimeError(f'mesh_project: V = {V} reaches the limit of 2^31')
    xy = torch.empty(V, 2, device=dev, dtype=torch.int32)
    z = torch.empty(V, device=dev, dtype=torch.float64)
    vflag = torch.empty(V, device=dev, dtype=torch.uint8)
    if V == 0:
        return xy, z, vflag
    with _guard(pos):
        rc = _lib.lib().occnerf_mesh_project(pp, V, K.ctypes.data_as(C.c_void_p), E.ctypes.data_as(C.c_void_p), xy.data_ptr(),
                                             z.data_ptr(), vflag.data_ptr(), _stream(pos))
    _lib.check(rc, 'mesh_project')
    return xy, z, vflag


def _mesh_raster_args(who, faces, xy, z, vflag, H, W):
    """vflag None: an entry that takes none (mesh_resolve_textured); its address comes back as None."""
    pf = _chk(faces, torch.int32, f'{who}: faces')
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError(f'{who}: faces must be int32 [T,3], got {tuple(faces.shape)}')
    px, pz = _chk(xy, torch.int32, f'{who}: xy'), _chk(z, torch.float64, f'{who}: z')
    pv = None if vflag is None else _chk(vflag, torch.uint8, f'{who}: vflag')
    V = int(z.numel())
    if tuple(xy.shape) != (V, 2) or z.dim() != 1 or not (xy.device == z.device == faces.device) or \
            (vflag is not None and (tuple(vflag.shape) != (V,) or vflag.device != faces.device)):
        raise RuntimeError(f"{who}: xy [V,2], z [V]{'' if vflag is None else ' and vflag [V]'} must be mesh_project's, on the device of faces")
    H, W = int(H), int(W)
    if not (1 <= H <= MESH_RASTER_MAX_SIDE and 1 <= W <= MESH_RASTER_MAX_SIDE and H * W <= MESH_RASTER_MAX_PIXELS):
        raise RuntimeError(f'{who}: H = {H}, W = {W} outside 1..{MESH_RASTER_MAX_SIDE} or more than 2^28 pixels')
    T = int(faces.shape[0])
    if T >= 1 << 31 or V >= 1 << 31:
        raise RuntimeError(f'{who}: T = {T} / V = {V} reaches the limit of 2^31')
    return pf, px, pz, pv, T, V, H, W


def _mesh_keys(who, keys):
    """mesh_raster's keys -> (address, H, W)."""
    pk = _chk(keys, torch.int64, f'{who}: keys')
    if keys.dim() != 2:
        raise RuntimeError(f'{who}: keys must be int64 [H,W], got {tuple(keys.shape)}')
    return pk, int(keys.shape[0]), int(keys.shape[1])


def mesh_raster(faces, xy, z, vflag, H, W, faces_checked=False):
    """Triangles into the per-pixel keys (occnerf_mesh_raster): faces int32 [T,3] and mesh_project's xy / z / vflag on one
    device -> (keys int64 [H,W]: the bits of (float32 depth) << 32 | triangle index of the nearest covering triangle, -1 (all
    ones) where there is none; counts int32 [7] in the order MESH_RASTER_COUNTS, 'covered' still 0).  A face index outside
    [0, V) is refused by name before anything is launched (one blocking read of the faces' extremes; faces_checked=True: the
    caller has made that test); the kernels themselves never use one as an address.  T = 0 or V = 0 launches nothing."""
    pf, px, pz, pv, T, V, H, W = _mesh_raster_args('mesh_raster', faces, xy, z, vflag, H, W)
    if T and not faces_checked:
        lo, hi = int(faces.min().item()), int(faces.max().item())
        if lo < 0 or hi >= V:
            raise RuntimeError(f'mesh_raster: face index {lo if lo < 0 else hi} outside [0, {V})')
    dev = faces.device
    keys = torch.full((H, W), -1, device=dev, dtype=torch.int64)
    counts = torch.zeros(len(MESH_RASTER_COUNTS), device=dev, dtype=torch.int32)
    if T == 0 or V == 0:
        return keys, counts
    wide_list = torch.empty(T, device=dev, dtype=torch.int32)
    with _guard(faces):
        rc = _lib.lib().occnerf_mesh_raster(pf, T, V, px, pz, pv, H, W, keys.data_ptr(), wide_list.data_ptr(), counts.data_ptr(),
                                            _stream(faces))
    _lib.check(rc, 'mesh_raster')
    return keys, counts


def mesh_resolve(keys, counts, faces, xy, z, vflag, colors, bgcolor):
    """The image of mesh_raster's keys (occnerf_mesh_resolve): colors uint8 [V,3] on the device, bgcolor 3 values 0..255 on the
    host -> (cover uint8 [H,W], tri int32 [H,W] (-1 empty), depth float32 [H,W] (+inf empty), rgb uint8 [H,W,3]); counts[6]
    receives the covered pixels.  T = 0 or V = 0 launches nothing: the empty image."""
    pk, H, W = _mesh_keys('mesh_resolve', keys)
    pf, px, pz, pv, T, V, H, W = _mesh_raster_args('mesh_resolve', faces, xy, z, vflag, H, W)
    pn = _chk(counts, torch.int32, 'mesh_resolve: counts')
    if counts.numel() != len(MESH_RASTER_COUNTS) or counts.device != faces.device or keys.device != faces.device:
        raise RuntimeError(f'mesh_resolve: keys and counts int32 [{len(MESH_RASTER_COUNTS)}] must be mesh_raster\'s')
    pc = _chk(colors, torch.uint8, 'mesh_resolve: colors')
    if tuple(colors.shape) != (V, 3) or colors.device != faces.device:
        raise RuntimeError(f'mesh_resolve: colors must be uint8 [{V},3] on the device of faces, got {tuple(colors.shape)}')
    bg = _mesh_bgcolor(bgcolor)
    dev = faces.device
    if T == 0 or V == 0:
        return (torch.zeros(H, W, device=dev, dtype=torch.uint8), torch.full((H, W), -1, device=dev, dtype=torch.int32),
                torch.full((H, W), float('inf'), device=dev, dtype=torch.float32),
                torch.from_numpy(bg).to(dev).expand(H, W, 3).contiguous())
    cover = torch.empty(H, W, device=dev, dtype=torch.uint8)
    tri = torch.empty(H, W, device=dev, dtype=torch.int32)
    depth = torch.empty(H, W, device=dev, dtype=torch.float32)
    rgb = torch.empty(H, W, 3, device=dev, dtype=torch.uint8)
    with _guard(faces):
        rc = _lib.lib().occnerf_mesh_resolve(pk, pf, T, V, px, pz, pv, pc, bg.ctypes.data_as(C.c_void_p), H, W, cover.data_ptr(),
                                             tri.data_ptr(), depth.data_ptr(), rgb.data_ptr(), pn, _stream(faces))
    _lib.check(rc, 'mesh_resolve')
    return cover, tri, depth, rgb


# ------------------------------------------------------------------ the texture of the exported mesh
MESH_TEXTURE_MIN_CELL, MESH_TEXTURE_MAX_CELL, MESH_TEXTURE_MAX_SIDE = 4, 64, 16384


def _mesh_texture_cell(who, n):
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or \
            not MESH_TEXTURE_MIN_CELL <= int(n) <= MESH_TEXTURE_MAX_CELL:
        raise RuntimeError(f'{who}: cell = {n!r} is not a whole number in {MESH_TEXTURE_MIN_CELL}..{MESH_TEXTURE_MAX_CELL}')
    return int(n)


def mesh_texture_layout(T, n, who='mesh_texture'):
    """(C, R, W, H, P) of the per-triangle atlas of T >= 1 triangles at cell edge n (4..64): ceil(T / 2) cells of n x n texels,
    C = ceil(sqrt(cells)) per row, R rows, W = C n, H = R n, P = n (n - 1) / 2 texels per triangle.  A cell edge out of range,
    T < 1 and W or H above 16384 are refused by name."""
    T, n = int(T), _mesh_texture_cell(who, n)
    if T < 1:
        raise RuntimeError(f'{who}: T = {T}: a mesh without triangles has no atlas')
    cells = (T + 1) // 2
    C = math.isqrt(cells - 1) + 1
    R = (cells + C - 1) // C
    W, H = C * n, R * n
    if W > MESH_TEXTURE_MAX_SIDE or H > MESH_TEXTURE_MAX_SIDE:
        raise RuntimeError(f'{who}: an atlas of {W} x {H} texels for {T} triangles at cell {n} exceeds {MESH_TEXTURE_MAX_SIDE} '
                           '(lower mesh_texture.cell or mesh.resolution)')
    return C, R, W, H, n * (n - 1) // 2


def _mesh_texel_args(who, verts, faces, n):
    """The mesh whose texels an entry walks: verts float32 [V,3], faces int32 [T,3] on its device, the cell edge n
    -> (address of verts, of faces, n, V, T, P = n (n - 1) / 2, device)."""
    n = _mesh_texture_cell(who, n)
    pv = _mesh_points(f'{who}: verts', verts)
    pf = _chk(faces, torch.int32, f'{who}: faces')
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.device != verts.device:
        raise RuntimeError(f'{who}: faces must be int32 [T,3] on the device of verts, got {tuple(faces.shape)}')
    V, T, P = int(verts.shape[0]), int(faces.shape[0]), n * (n - 1) // 2
    if V >= 1 << 31 or T * P >= 1 << 31:
        raise RuntimeError(f'{who}: V = {V} or T P = {T} x {P} reaches the limit of 2^31')
    return pv, pf, n, V, T, P, verts.device


def _mesh_face_status(who, status, V):
    """One blocking read of a kernel's status word."""
    if int(status.item()) != 0:
        raise RuntimeError(f'{who}: a face index lies outside [0, {V})')


def mesh_texel_points(verts, faces, n):
    """The canonical points of the atlas' texels (occnerf_mesh_texel_points): verts float32 [V,3], faces int32 [T,3], n the cell
    edge -> pts float32 [T,P,3], P = n (n - 1) / 2, on the device of verts.  A face index outside [0, V) is refused by name
    after one blocking read of the kernel's status word (the kernel itself never uses one as an address).  T = 0 launches
    nothing."""
    pv, pf, n, V, T, P, dev = _mesh_texel_args('mesh_texel_points', verts, faces, n)
    pts = torch.empty(T, P, 3, device=dev, dtype=torch.float32)
    if T == 0:
        return pts
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    with _guard(verts):
        rc = _lib.lib().occnerf_mesh_texel_points(pv, V, pf, T, n, pts.data_ptr(), status.data_ptr(), _stream(verts))
    _lib.check(rc, 'mesh_texel_points')
    _mesh_face_status('mesh_texel_points', status, V)
    return pts


def _mesh_texture_atlas(who, atlas, T, n, C, dev):
    pa = _chk(atlas, torch.uint8, f'{who}: atlas')
    if atlas.dim() != 3 or atlas.shape[2] != 3 or atlas.device != dev:
        raise RuntimeError(f'{who}: atlas must be uint8 [H,W,3] on the device of the other tensors, got {tuple(atlas.shape)}')
    H, W, C = int(atlas.shape[0]), int(atlas.shape[1]), int(C)
    rows = (((T + 1) // 2) + C - 1) // C if C >= 1 else 0
    if C < 1 or W != C * n or rows * n > H or H > MESH_TEXTURE_MAX_SIDE or W > MESH_TEXTURE_MAX_SIDE:
        raise RuntimeError(f'{who}: an atlas of H = {H}, W = {W} with C = {C} cells of {n} per row does not hold T = {T} triangles '
                           f'(W = C n, {rows} rows of cells, at most {MESH_TEXTURE_MAX_SIDE} texels a side)')
    return pa, H, W, C


def mesh_texture_fill(rgb, T, n, C, atlas):
    """The queried colours as bytes at their places in the atlas (occnerf_mesh_texture_fill): rgb float32 [T P,3] in the order
    of mesh_texel_points' rows, atlas uint8 [H,W,3] with W = C n, filled by the caller, written IN PLACE -> atlas.  Only owned
    texels are written: image.to_8b_image's rule, 0 for a NaN.  T = 0 launches nothing."""
    n = _mesh_texture_cell('mesh_texture_fill', n)
    pr = _chk(rgb, torch.float32, 'mesh_texture_fill: rgb')
    T, P = int(T), n * (n - 1) // 2
    if T < 0 or T * P >= 1 << 31 or tuple(rgb.shape) != (T * P, 3):
        raise RuntimeError(f'mesh_texture_fill: rgb must be float32 [{T} x {P},3] with T P < 2^31, got {tuple(rgb.shape)}')
    pa, H, W, C = _mesh_texture_atlas('mesh_texture_fill', atlas, T, n, C, rgb.device)
    if T == 0:
        return atlas
    with _guard(rgb):
        rc = _lib.lib().occnerf_mesh_texture_fill(pr, T, n, C, H, W, pa, _stream(rgb))
    _lib.check(rc, 'mesh_texture_fill')
    return atlas


def mesh_resolve_textured(keys, faces, xy, z, atlas, n, C, bgcolor):
    """The textured image of mesh_raster's keys (occnerf_mesh_resolve_textured), the twin of mesh_resolve: keys int64 [H,W],
    faces int32 [T,3], mesh_project's xy / z, atlas uint8 [aH,aW,3] of cell edge n with C cells per row, bgcolor 3 values
    0..255 on the host -> rgb uint8 [H,W,3].  The winner's four taps are its own texels.  No triangle: the background."""
    n = _mesh_texture_cell('mesh_resolve_textured', n)
    pk, H, W = _mesh_keys('mesh_resolve_textured', keys)
    pf, px, pz, _, T, V, H, W = _mesh_raster_args('mesh_resolve_textured', faces, xy, z, None, H, W)
    dev = faces.device
    if keys.device != dev:
        raise RuntimeError('mesh_resolve_textured: keys must be mesh_raster\'s, on the device of faces')
    pa, aH, aW, C = _mesh_texture_atlas('mesh_resolve_textured', atlas, T, n, C, dev)
    bg = _mesh_bgcolor(bgcolor)
    rgb = torch.empty(H, W, 3, device=dev, dtype=torch.uint8)
    with _guard(faces):
        rc = _lib.lib().occnerf_mesh_resolve_textured(pk, pf, T, V, px, pz, H, W, pa, aH, aW, n, C, bg.ctypes.data,
                                                      rgb.data_ptr(), _stream(faces))
    _lib.check(rc, 'mesh_resolve_textured')
    return rgb


# ------------------------------------------------------------------ the normal map of the exported mesh
MESH_NORMAL_MAX_STEPS = 64
MESH_NORMAL_FLAGS = {'no_crossing': 1, 'no_gradient': 2, 'flat': 4, 'face_direction': 8}
MESH_NORMAL_FLAT = (128, 128, 255)


def mesh_normal_steps(cage, h_f, who='mesh_normal_bake'):
    """S = ceil(cage / (h_f / 2)), the steps of half a fine voxel to either side of a texel; S outside 1..64 is refused by name."""
    cage, h_f = float(cage), float(h_f)
    if not (0.0 < h_f < float('inf')) or not (0.0 < cage < float('inf')):
        raise RuntimeError(f'{who}: cage = {cage!r} and h_f = {h_f!r} must be positive finite lengths')
    S = int(math.ceil(cage / (h_f / 2.0)))
    if not 1 <= S <= MESH_NORMAL_MAX_STEPS:
        raise RuntimeError(f'{who}: cage = {cage!r} at a fine voxel of {h_f!r} takes S = {S} steps, outside 1..{MESH_NORMAL_MAX_STEPS} '
                           '(lower mesh_normal.cage or mesh_normal.resolution)')
    return S


def mesh_normal_bake(verts, vnormals, faces, tangents, creased, pts, n, C, atlas, field, lo, h_f, level, S):
    """The normal map's texels (occnerf_mesh_normal_bake): verts / vnormals float32 [V,3], faces int32 [T,3], tangents float32
    [T,3,4] and creased uint8 [T] (mesh.corner_tangents), pts float32 [T,P,3] (mesh_texel_points), atlas uint8 [H,W,3] with
    W = C n, filled by the caller with the flat code and written IN PLACE, field float32 [nz,ny,nx] with grid point (i,j,k) at
    lo + (i,j,k) h_f (lo: 3 host values, float64), level the iso-value (float32), S the steps of h_f / 2 to either side
    -> (atlas, offset float32 [T,P], flags uint8 [T,P], normal float32 [T,P,3]).  A face index outside [0, V) is refused by
    name after one blocking read of the kernel's status word (the kernel itself never uses one as an address).  T = 0 launches
    nothing."""
    pv, pf, n, V, T, P, dev = _mesh_texel_args('mesh_normal_bake', verts, faces, n)
    pn = _mesh_points('mesh_normal_bake: vnormals', vnormals)
    if tuple(vnormals.shape) != (V, 3) or vnormals.device != dev:
        raise RuntimeError(f'mesh_normal_bake: vnormals must be float32 [{V},3] on the device of verts, got {tuple(vnormals.shape)}')
    pt = _chk(tangents, torch.float32, 'mesh_normal_bake: tangents')
    pc = _chk(creased, torch.uint8, 'mesh_normal_bake: creased')
    pp = _chk(pts, torch.float32, 'mesh_normal_bake: pts')
    if tuple(tangents.shape) != (T, 3, 4) or tuple(creased.shape) != (T,) or tuple(pts.shape) != (T, P, 3) or \
            not (tangents.device == creased.device == pts.device == dev):
        raise RuntimeError(f'mesh_normal_bake: tangents [{T},3,4], creased [{T}] and pts [{T},{P},3] must lie on the device of verts, '
                           f'got {tuple(tangents.shape)}, {tuple(creased.shape)} and {tuple(pts.shape)}')
    pa, H, W, C = _mesh_texture_atlas('mesh_normal_bake', atlas, T, n, C, dev)
    pg, nx, ny, nz = _mesh_field('mesh_normal_bake', field)
    if field.device != dev:
        raise RuntimeError('mesh_normal_bake: field must lie on the device of verts')
    lo = np.ascontiguousarray(np.asarray(lo, dtype=np.float64).reshape(3))
    h_f, S = float(h_f), int(S)
    if not (0.0 < h_f < float('inf')) or not np.all(np.isfinite(lo)):
        raise RuntimeError(f'mesh_normal_bake: lo = {lo.tolist()} / h_f = {h_f!r}: a finite corner and a positive finite voxel edge are needed')
    if not 1 <= S <= MESH_NORMAL_MAX_STEPS:
        raise RuntimeError(f'mesh_normal_bake: S = {S} steps outside 1..{MESH_NORMAL_MAX_STEPS}')
    offset = torch.empty(T, P, device=dev, dtype=torch.float32)
    flags = torch.empty(T, P, device=dev, dtype=torch.uint8)
    normal = torch.empty(T, P, 3, device=dev, dtype=torch.float32)
    if T == 0:
        return atlas, offset, flags, normal
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    with _guard(verts):
        rc = _lib.lib().occnerf_mesh_normal_bake(pv, pn, V, pf, T, pt, pc, pp, n, C, H, W, pg, nx, ny, nz, lo.ctypes.data, h_f,
                                                 float(np.float32(level)), S, pa, offset.data_ptr(), flags.data_ptr(),
                                                 normal.data_ptr(), status.data_ptr(), _stream(verts))
    _lib.check(rc, 'mesh_normal_bake')
    _mesh_face_status('mesh_normal_bake', status, V)
    return atlas, offset, flags, normal


def mesh_ray_matrix(K, E):
    """float64 3x3 M with M (column, row, 1) the ray direction of a pixel in the space E looks at: R^T K^-1 of K 3x3 and
    E = [R | t] 4x4 on the host."""
    K, E = _host_matrix64(K, (3, 3), 'mesh_ray_matrix: K'), _host_matrix64(E, (4, 4), 'mesh_ray_matrix: E')
    return np.ascontiguousarray(E[:3, :3].T @ np.linalg.inv(K))


def mesh_resolve_lit(keys, faces, xy, z, vnormals, tangents, atlas, n, C, M, bgcolor):
    """Two headlight panels of mesh_raster's keys (occnerf_mesh_resolve_lit): keys int64 [H,W], faces int32 [T,3], mesh_project's
    xy / z, vnormals float32 [V,3] and tangents float32 [T,3,4] of the posed mesh, the normal atlas uint8 [aH,aW,3] of cell edge
    n with C cells per row, M 3x3 float64 on the host (mesh_ray_matrix), bgcolor 3 values 0..255 on the host
    -> (shade_geometry, shade_mapped) uint8 [H,W,3]: the interpolated vertex normal alone, and the normal the atlas gives in
    the frame a glTF viewer reconstructs.  No triangle: the background."""
    n = _mesh_texture_cell('mesh_resolve_lit', n)
    pk, H, W = _mesh_keys('mesh_resolve_lit', keys)
    pf, px, pz, _, T, V, H, W = _mesh_raster_args('mesh_resolve_lit', faces, xy, z, None, H, W)
    dev = faces.device
    if keys.device != dev:
        raise RuntimeError('mesh_resolve_lit: keys must be mesh_raster\'s, on the device of faces')
    pn = _mesh_points('mesh_resolve_lit: vnormals', vnormals)
    pt = _chk(tangents, torch.float32, 'mesh_resolve_lit: tangents')
    if tuple(vnormals.shape) != (V, 3) or tuple(tangents.shape) != (T, 3, 4) or vnormals.device != dev or tangents.device != dev:
        raise RuntimeError(f'mesh_resolve_lit: vnormals [{V},3] and tangents [{T},3,4] must lie on the device of faces, got '
                           f'{tuple(vnormals.shape)} and {tuple(tangents.shape)}')
    pa, aH, aW, C = _mesh_texture_atlas('mesh_resolve_lit', atlas, T, n, C, dev)
    M = _host_matrix64(M, (3, 3), 'mesh_resolve_lit: M')
    bg = _mesh_bgcolor(bgcolor)
    geometry = torch.empty(H, W, 3, device=dev, dtype=torch.uint8)
    mapped = torch.empty(H, W, 3, device=dev, dtype=torch.uint8)
    with _guard(faces):
        rc = _lib.lib().occnerf_mesh_resolve_lit(pk, pf, T, V, px, pz, H, W, pn, pt, pa, aH, aW, n, C, M.ctypes.data,
                                                 bg.ctypes.data, geometry.data_ptr(), mapped.data_ptr(), _stream(faces))
    _lib.check(rc, 'mesh_resolve_lit')
    return geometry, mapped


# ------------------------------------------------------------------ the photographs on the atlas
def mesh_texture_project(xy, z, vflag, verts, pflag, faces, n, K, E, keys, photo, inside, bias, acc, seen):
    """One frame onto the atlas' accumulators (occnerf_mesh_texture_project): xy int32 [T P,2] / z float64 [T P] / vflag uint8
    [T P] are mesh_project's of mesh_texel_points(verts, faces, n); verts float32 [V,3] the posed vertices, pflag uint8 [V]
    their posing flags, faces int32 [T,3]; K 3x3 and E 4x4 on the host as mesh_project takes them; keys int64 [H,W]
    mesh_raster's of the same verts and faces; photo uint8 [H,W,3], inside uint8 [H,W]; bias >= 0 in metres; acc int64 [T P,4]
    and seen int32 [T P] are written IN PLACE -> tri_w int32 [T]: the triangles' weights in this frame, 1..256, 0 unusable,
    -1 facing away.  A face index outside [0, V) is refused by name after one blocking read of the status word (no such index
    is used as an address).  T = 0 launches nothing."""
    who = 'mesh_texture_project'
    pv, pf, n, V, T, P, dev = _mesh_texel_args(who, verts, faces, n)
    pp = _chk(pflag, torch.uint8, f'{who}: pflag')
    N = T * P
    px, pz, pw = _chk(xy, torch.int32, f'{who}: xy'), _chk(z, torch.float64, f'{who}: z'), _chk(vflag, torch.uint8, f'{who}: vflag')
    (pk, H, W), ph, pi = _mesh_keys(who, keys), _chk(photo, torch.uint8, f'{who}: photo'), _chk(inside, torch.uint8, f'{who}: inside')
    pa, ps = _chk(acc, torch.int64, f'{who}: acc'), _chk(seen, torch.int32, f'{who}: seen')
    if tuple(pflag.shape) != (V,) or tuple(xy.shape) != (N, 2) or tuple(z.shape) != (N,) or tuple(vflag.shape) != (N,):
        raise RuntimeError(f'{who}: pflag must be [{V}] and xy / z / vflag [{N},2] / [{N}] / [{N}], got {tuple(pflag.shape)}, '
                           f'{tuple(xy.shape)}, {tuple(z.shape)}, {tuple(vflag.shape)}')
    if not (1 <= H <= MESH_RASTER_MAX_SIDE and 1 <= W <= MESH_RASTER_MAX_SIDE):
        raise RuntimeError(f'{who}: H = {H}, W = {W} outside 1..{MESH_RASTER_MAX_SIDE}')
    if tuple(photo.shape) != (H, W, 3) or tuple(inside.shape) != (H, W):
        raise RuntimeError(f'{who}: photo must be uint8 [{H},{W},3] and inside uint8 [{H},{W}], got {tuple(photo.shape)} and '
                           f'{tuple(inside.shape)}')
    if tuple(acc.shape) != (N, 4) or tuple(seen.shape) != (N,):
        raise RuntimeError(f'{who}: acc must be int64 [{N},4] and seen int32 [{N}], got {tuple(acc.shape)} and {tuple(seen.shape)}')
    if not all(t.device == dev for t in (pflag, xy, z, vflag, keys, photo, inside, acc, seen)):
        raise RuntimeError(f'{who}: every tensor must be on the device of verts')
    K, E = _host_matrix64(K, (3, 3), f'{who}: K'), _host_matrix64(E, (4, 4), f'{who}: E')
    if K[0, 1] != 0.0:
        raise NotImplementedError(f'{who}: skew K[0,1] = {K[0, 1]!r} is not built')
    bias = float(bias)
    if not bias >= 0.0:
        raise RuntimeError(f'{who}: bias = {bias!r} is negative or not a number')
    tri_w = torch.zeros(T, device=dev, dtype=torch.int32)
    if T == 0:
        return tri_w
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    with _guard(verts):
        rc = _lib.lib().occnerf_mesh_texture_project(px, pz, pw, pv, pp, V, pf, T, n, K.ctypes.data_as(C.c_void_p),
                                                     E.ctypes.data_as(C.c_void_p), pk, ph, pi, H, W, bias, pa, ps,
                                                     tri_w.data_ptr(), status.data_ptr(), _stream(verts))
    _lib.check(rc, who)
    _mesh_face_status(who, status, V)
    return tri_w


def mesh_texture_blend(acc, seen, T, n, C, atlas, min_seen=1):
    """The accumulators as an atlas (occnerf_mesh_texture_blend): acc int64 [T P,4], seen int32 [T P], atlas uint8 [H,W,3] the
    field's (mesh_texture_fill's; not written) -> (photo uint8 [H,W,3], seen_img uint8 [H,W]): an owned texel with
    seen >= min_seen carries (acc_c + 32768 acc_3) // (65536 acc_3), every other texel atlas' byte; seen_img holds
    min(seen, 255) at the owned texels and 0 elsewhere.  T = 0 launches nothing."""
    who = 'mesh_texture_blend'
    n = _mesh_texture_cell(who, n)
    pa, ps = _chk(acc, torch.int64, f'{who}: acc'), _chk(seen, torch.int32, f'{who}: seen')
    T, P = int(T), n * (n - 1) // 2
    if T < 0 or T * P >= 1 << 31 or tuple(acc.shape) != (T * P, 4) or tuple(seen.shape) != (T * P,) or seen.device != acc.device:
        raise RuntimeError(f'{who}: acc must be int64 [{T} x {P},4] and seen int32 [{T} x {P}] with T P < 2^31 on one device, got '
                           f'{tuple(acc.shape)} and {tuple(seen.shape)}')
    if isinstance(min_seen, (bool, np.bool_)) or not isinstance(min_seen, (int, np.integer)) or not 1 <= int(min_seen) < 1 << 31:
        raise RuntimeError(f'{who}: min_seen = {min_seen!r} is not a whole number >= 1')
    _, H, W, C = _mesh_texture_atlas(who, atlas, T, n, C, acc.device)
    out = atlas.clone()
    seen_img = torch.zeros(H, W, device=acc.device, dtype=torch.uint8)
    if T == 0:
        return out, seen_img
    with _guard(acc):
        rc = _lib.lib().occnerf_mesh_texture_blend(pa, ps, T, n, C, H, W, int(min_seen), out.data_ptr(), seen_img.data_ptr(),
                                                   _stream(acc))
    _lib.check(rc, who)
    return out, seen_img


# ------------------------------------------------------------------ geometry maps of a rendered frame
GBUFFER_PANELS = ('depth', 'normal', 'shaded')
GBUFFER_MAX_PIXELS = 1 << 31


def _gbuffer_rays(who, rays, dev):
    pr = _chk(rays, torch.float32, f'{who}: rays')
    if rays.dim() != 3 or rays.shape[0] != 2 or rays.shape[2] != 3 or rays.device != dev:
        raise RuntimeError(f'{who}: rays must be float32 [2,R,3] on {dev}, got {tuple(rays.shape)} on {rays.device}')
    return pr, int(rays.shape[1])


def gbuffer_points(ray_index, rays, depth, alpha, min_alpha, height, width):
    """The surface point of every pixel's ray (occnerf_gbuffer_points): ray_index int64 [R] ascending flat pixels, rays float32
    [2,R,3], depth / alpha float32 [R] on one device -> (points float32 [H,W,4]: o + t d and t = depth / alpha, zeros where the
    pixel has no ray or alpha < min_alpha, alpha <= 0 or a value is not finite; valid uint8 [H,W]: bit 0; pix_ray int32 [H,W]:
    the ray's row, -1 where not valid)."""
    H, W = int(height), int(width)
    if H <= 0 or W <= 0 or H * W >= GBUFFER_MAX_PIXELS:
        raise RuntimeError(f'gbuffer_points: height = {H}, width = {W} must be positive with fewer than 2^31 pixels')
    pi = _chk(ray_index, torch.int64, 'gbuffer_points: ray_index')
    dev = ray_index.device
    pr, R = _gbuffer_rays('gbuffer_points', rays, dev)
    pd, pa = _chk(depth, torch.float32, 'gbuffer_points: depth'), _chk(alpha, torch.float32, 'gbuffer_points: alpha')
    if tuple(ray_index.shape) != (R,) or tuple(depth.shape) != (R,) or tuple(alpha.shape) != (R,) or \
            not (depth.device == alpha.device == dev):
        raise RuntimeError(f'gbuffer_points: ray_index, depth and alpha must be [{R}] like rays, on {dev}; got '
                           f'{tuple(ray_index.shape)}, {tuple(depth.shape)}, {tuple(alpha.shape)}')
    if R > H * W:
        raise RuntimeError(f'gbuffer_points: R = {R} is larger than height * width = {H * W}')
    points = torch.empty(H, W, 4, device=dev, dtype=torch.float32)
    valid = torch.empty(H, W, device=dev, dtype=torch.uint8)
    pix_ray = torch.empty(H, W, device=dev, dtype=torch.int32)
    with _guard_dev(dev):
        rc = _lib.lib().occnerf_gbuffer_points(pi if R else None, R, pr if R else None, pd if R else None, pa if R else None,
                                               float(min_alpha), H, W, points.data_ptr(), valid.data_ptr(), pix_ray.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, 'gbuffer_points')
    return points, valid, pix_ray


def gbuffer_normals(points, pix_ray, rays, t_range, bgcolor01, panels=GBUFFER_PANELS, valid=None):
    """Normals from the point map's secants, and the panels (occnerf_gbuffer_normals): points / pix_ray of gbuffer_points and
    the same rays; t_range float32 [2] ON THE DEVICE (t_lo, t_hi), None allowed without the depth panel; bgcolor01: 3 host
    floats -> (normal float32 [H,W,3], valid uint8 [H,W] with bit 0 depth-valid and bit 1 normal valid, {name: uint8 [H,W,3]}
    for the names in `panels`, a subset of GBUFFER_PANELS).  valid: gbuffer_points' uint8 [H,W] to finish in place (every
    thread writes its own byte whole and reads none); None allocates one."""
    pp = _chk(points, torch.float32, 'gbuffer_normals: points')
    if points.dim() != 3 or points.shape[2] != 4:
        raise RuntimeError(f'gbuffer_normals: points must be float32 [H,W,4], got {tuple(points.shape)}')
    H, W = int(points.shape[0]), int(points.shape[1])
    if H <= 0 or W <= 0 or H * W >= GBUFFER_MAX_PIXELS:
        raise RuntimeError(f'gbuffer_normals: height = {H}, width = {W} must be positive with fewer than 2^31 pixels')
    dev = points.device
    pq = _chk(pix_ray, torch.int32, 'gbuffer_normals: pix_ray')
    if tuple(pix_ray.shape) != (H, W) or pix_ray.device != dev:
        raise RuntimeError(f'gbuffer_normals: pix_ray must be int32 [{H},{W}] on {dev}, got {tuple(pix_ray.shape)} on {pix_ray.device}')
    pr, R = _gbuffer_rays('gbuffer_normals', rays, dev)
    if R > H * W:
        raise RuntimeError(f'gbuffer_normals: R = {R} is larger than height * width = {H * W}')
    panels = tuple(panels)
    unknown = [k for k in panels if k not in GBUFFER_PANELS]
    if unknown:
        raise RuntimeError(f'gbuffer_normals: unknown panel {unknown[0]!r}; the panels are {GBUFFER_PANELS}')
    pt = None
    if 'depth' in panels:
        if t_range is None:
            raise RuntimeError('gbuffer_normals: the depth panel needs t_range')
        pt = _chk(t_range, torch.float32, 'gbuffer_normals: t_range')
        if t_range.numel() != 2 or t_range.device != dev:
            raise RuntimeError(f'gbuffer_normals: t_range must be float32 [2] on {dev}, got {tuple(t_range.shape)} on {t_range.device}')
    _bg, pbg = _host_f32(bgcolor01, 3)
    normal = torch.empty(H, W, 3, device=dev, dtype=torch.float32)
    if valid is None:
        valid = torch.empty(H, W, device=dev, dtype=torch.uint8)
    else:
        _chk(valid, torch.uint8, 'gbuffer_normals: valid')
        if tuple(valid.shape) != (H, W) or valid.device != dev:
            raise RuntimeError(f'gbuffer_normals: valid must be uint8 [{H},{W}] on {dev}, got {tuple(valid.shape)} on {valid.device}')
    out = {k: torch.empty(H, W, 3, device=dev, dtype=torch.uint8) for k in GBUFFER_PANELS if k in panels}
    ptr = {k: (out[k].data_ptr() if k in out else None) for k in GBUFFER_PANELS}
    with _guard_dev(dev):
        rc = _lib.lib().occnerf_gbuffer_normals(pp, pq, pr if R else None, R, H, W, pt, pbg, normal.data_ptr(), valid.data_ptr(),
                                                ptr['depth'], ptr['normal'], ptr['shaded'],
                                                torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, 'gbuffer_normals')
    return normal, valid, out


# ------------------------------------------------------------------ the driving skeleton of an animate frame
SKELETON_JOINTS = 24


def skeleton_panel(joints, K, E, height, width, bone_px, palette, bgcolor_u8, device):
    """The skeleton panel of one frame (occnerf_skeleton_panel): joints [24,3] float32 in the space of the rays, K [3,3] and E
    [4,4] (taken as float64), bone_px the half-width of a bone in pixels, palette uint8 [24,3], bgcolor_u8 3 bytes -- all on the
    HOST, taken by value -> (img uint8 [H,W,3], record int32 [1 + workgroups]) on `device`: record[0] the joints dropped,
    record[1:] the pixels each workgroup covered.  One launch on the current stream; nothing synchronises."""
    H, W = int(height), int(width)
    if H < 1 or W < 1 or H * W >= GBUFFER_MAX_PIXELS:
        raise RuntimeError(f'skeleton_panel: height = {H}, width = {W} must be positive with fewer than 2^31 pixels')
    j = np.ascontiguousarray(np.asarray(joints))
    if j.shape != (SKELETON_JOINTS, 3) or j.dtype != np.float32:
        raise RuntimeError(f'skeleton_panel: joints must be float32 [{SKELETON_JOINTS},3], got {j.dtype} {j.shape}')
    K = np.ascontiguousarray(np.asarray(K, dtype=np.float64)[:3, :3])
    E = np.ascontiguousarray(np.asarray(E, dtype=np.float64))
    if K.shape != (3, 3) or E.shape != (4, 4):
        raise RuntimeError(f'skeleton_panel: K must be [3,3] and E [4,4], got {K.shape} and {E.shape}')
    if K[0, 1] != 0.0:
        raise NotImplementedError(f'skeleton_panel: skew K[0,1] = {K[0, 1]!r} is not built')
    r = float(bone_px)
    if not 0.0 <= r <= 1.0e6:
        raise RuntimeError(f'skeleton_panel: bone_px = {bone_px!r} outside 0..1e6')
    pal = np.ascontiguousarray(np.asarray(palette))
    bg = np.ascontiguousarray(np.asarray(bgcolor_u8))
    if pal.shape != (SKELETON_JOINTS, 3) or pal.dtype != np.uint8 or bg.shape != (3,) or bg.dtype != np.uint8:
        raise RuntimeError(f'skeleton_panel: palette must be uint8 [{SKELETON_JOINTS},3] and bgcolor_u8 uint8 [3], got '
                           f'{pal.dtype} {pal.shape} and {bg.dtype} {bg.shape}')
    dev = torch.device(device)
    blocks = int(_lib.lib().occnerf_skeleton_panel_blocks(H, W))
    with _guard_dev(dev):
        img = torch.empty(H, W, 3, device=dev, dtype=torch.uint8)
        record = torch.empty(1 + blocks, device=dev, dtype=torch.int32)
        rc = _lib.lib().occnerf_skeleton_panel(j.ctypes.data, K.ctypes.data, E.ctypes.data, r, pal.ctypes.data, bg.ctypes.data,
                                               H, W, img.data_ptr(), record.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, 'skeleton_panel')
    return img, record
