"""Image metrics of the reference's eval.py (eval.py:100-218) on the GPU: SSIM, PSNR over the vis / body / full pixel
selections and the silhouette IoU, from one HIP launch pair per batch of frames (csrc/metrics.hip).

The metric is eval.py's, quirks included:
  * images: the 8-bit images unpack_to_image builds (background cfg.bgcolor, to_8b_image truncation), divided by 255 in
    float64 -- metrics are taken on the quantised pixels, not on the float rays;
  * SSIM: skimage.metrics.structural_similarity(pred, truth, multichannel=True, full=True) on those float64 images.  It is
    restated from skimage's source (no skimage here): 7x7 uniform window, scipy's 'reflect' border, sample covariance
    (49/48), K1 = 0.01, K2 = 0.03, and data_range = 2 because skimage takes it from float64's dtype range (-1, 1).  mssim
    ("SSIM-full") is the mean over channels of S with 3 pixels cropped from each edge; the masked SSIMs are means of the
    uncropped S over the selected pixels, all three channels;
  * masks, compared in float32 as numpy does: body = ray_mask; vis = alpha > 0.001 (or gt ray_alpha > 0.5 when the frame
    carries ray_alpha); IoU = (alpha > 0.1) against (gt alpha > 0.5);
  * PSNR = -10 log(mse) / log(10) over the selected elements; an empty selection gives nan and a zero error inf, as numpy
    does.  (eval.py appends IOU twice per frame; the mean it prints is the same as with one entry per frame.)

The kernel forms the 7x7 box sums of x, y, x^2, y^2 and xy as exact integers and evaluates S in fp64 from them, so
identical images give S == 1.0 bit for bit and every sum is formed in a fixed order (bitwise deterministic).
"""
import numpy as np
import torch

from . import _lib, ops

RECORD = 14               # include/occnerf_hip.h OCCNERF_FRAME_METRICS_RECORD
KEYS = ('psnr_vis', 'ssim_vis', 'psnr_body', 'ssim_body', 'psnr_full', 'ssim_full', 'iou')
WIN_SIZE = 7


def _opt(t, dtype, name):
    return None if t is None else ops._chk(t, dtype, name)


def _frame_metrics_raw(pred, truth, alpha=None, body=None, gt_vis=None, gt_alpha=None, data_range=2.0, want_map=False):
    """pred, truth uint8 [N,H,W,3] (or [H,W,3]) on the GPU; alpha / gt_vis / gt_alpha float32 and body uint8 [N,H,W]
    (or [H,W]), each optional -> (record float64 [N, RECORD] on the GPU, S map float64 [N,H,W,3] or None)."""
    if pred.dim() == 3:
        pred, truth = pred[None], truth[None]
        alpha, body, gt_vis, gt_alpha = (None if t is None else t[None] for t in (alpha, body, gt_vis, gt_alpha))
    if pred.shape != truth.shape or pred.dim() != 4 or pred.shape[-1] != 3:
        raise ValueError(f'frame metrics: images must both be [N,H,W,3], got {tuple(pred.shape)} and {tuple(truth.shape)}')
    N, H, W = (int(s) for s in pred.shape[:3])
    for t, name in ((alpha, 'alpha'), (body, 'body'), (gt_vis, 'gt_vis'), (gt_alpha, 'gt_alpha')):
        if t is not None and tuple(t.shape) != (N, H, W):
            raise ValueError(f'frame metrics: {name} must be [{N},{H},{W}], got {tuple(t.shape)}')
    if H < WIN_SIZE or W < WIN_SIZE:
        raise ValueError(f'frame metrics: images of {H}x{W}: SSIM needs at least {WIN_SIZE} pixels on each side, as skimage')
    dev = pred.device
    ws = int(_lib.lib().occnerf_frame_metrics_workspace_bytes(N, H, W))
    if ws < 0:
        raise ValueError(f'frame metrics: {N} frames of {H}x{W} are not supported')
    work = torch.empty(ws, device=dev, dtype=torch.uint8)
    record = torch.empty(N, RECORD, device=dev, dtype=torch.float64)
    smap = torch.empty(N, H, W, 3, device=dev, dtype=torch.float64) if want_map else None
    with ops._guard_dev(dev):
        rc = _lib.lib().occnerf_frame_metrics(
            ops._chk(pred, torch.uint8, 'pred'), ops._chk(truth, torch.uint8, 'truth'), _opt(alpha, torch.float32, 'alpha'),
            _opt(body, torch.uint8, 'body'), _opt(gt_vis, torch.float32, 'gt_vis'), _opt(gt_alpha, torch.float32, 'gt_alpha'),
            N, H, W, float(data_range), record.data_ptr(), None if smap is None else smap.data_ptr(), work.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, 'frame_metrics')
    return record, smap


def _as_uint8(im, name):
    """GPU uint8 [H,W,3] as it is; a float image only if it holds exact multiples of 1/255 in [0, 1] (eval.py's x / 255.)."""
    if not torch.is_tensor(im) or not im.is_cuda:
        raise TypeError(f'{name}: a GPU tensor is required (there is no host path)')
    if im.dtype == torch.uint8:
        return im.contiguous()
    if not im.is_floating_point():
        raise TypeError(f'{name}: uint8 or floating point expected, got {im.dtype}')
    q = torch.round(im.double() * 255.)
    if bool(((q < 0) | (q > 255)).any()) or not torch.equal((q / 255.).to(im.dtype), im):
        raise ValueError(f'{name}: a float image must hold exact multiples of 1/255 in [0, 1] (8-bit pixels / 255.)')
    return q.to(torch.uint8).contiguous()


def structural_similarity(im1, im2, *, win_size=None, gradient=False, data_range=None, multichannel=True,
                          gaussian_weights=False, full=False, **kwargs):
    """skimage.metrics.structural_similarity as eval.py calls it (float64 images x / 255., multichannel=True), on the GPU.

    im1, im2: [H,W,3] GPU tensors, uint8 (the pixel values, read as x / 255.) or floating point holding exact multiples
    of 1/255 (anything else is refused).  data_range: in units of x / 255; None -> 2.0, what skimage derives from the float64
    dtype range.  Returns mssim (a float) and, with full=True, (mssim, S) with S the float64 [H,W,3] map on the GPU.
    Only what eval.py uses is built: gaussian_weights, a win_size other than 7, gradient, use_sample_covariance=False and
    other K1 / K2 / sigma are refused by name."""
    if gradient:
        raise NotImplementedError('structural_similarity: gradient=True is not built')
    if gaussian_weights:
        raise NotImplementedError('structural_similarity: gaussian_weights=True is not built (uniform 7x7 window only)')
    if win_size not in (None, WIN_SIZE):
        raise NotImplementedError(f'structural_similarity: win_size={win_size} is not built (7 only)')
    if not multichannel:
        raise NotImplementedError('structural_similarity: multichannel=False is not built ([H,W,3] images only)')
    for k, default in (('use_sample_covariance', True), ('K1', 0.01), ('K2', 0.03)):
        if k in kwargs and kwargs.pop(k) != default:
            raise NotImplementedError(f'structural_similarity: {k} other than {default} is not built')
    if kwargs:
        raise NotImplementedError(f'structural_similarity: {", ".join(sorted(kwargs))} not built')
    a, b = _as_uint8(im1, 'im1'), _as_uint8(im2, 'im2')
    if a.shape != b.shape or a.dim() != 3 or a.shape[-1] != 3:
        raise ValueError(f'structural_similarity: images must both be [H,W,3], got {tuple(a.shape)} and {tuple(b.shape)}')
    record, smap = _frame_metrics_raw(a, b, data_range=2.0 if data_range is None else data_range, want_map=full)
    mssim = float(record[0, 5].item())
    return (mssim, smap[0]) if full else mssim


def pixel_map(ray_index, values, height, width, dtype=None):
    """values[R] scattered into an [H,W] map by ray_index (flat pixel index of every ray), 0 elsewhere: eval.py's
    unpack_alpha_map (and its gt_mask / body_mask construction) on the device."""
    out = torch.zeros(height * width, device=values.device, dtype=dtype or values.dtype)
    out[ray_index] = values.to(out.dtype)
    return out.view(height, width)


def frame_metrics(rgb, alpha, ray_index, target_rgb, width, height, *, ray_alpha=None, gt_alpha=None,
                  bgcolor=(1., 1., 1.), data_range=2.0, with_images=False):
    """eval.py:140-196 for one frame on the GPU.  rgb [R,3], alpha [R] (the renderer's output), ray_index int64 [R]
    (ascending flat pixel index of every ray, nonzero(ray_mask)), target_rgb [R,3]; ray_alpha [R] or [R,k] (column 0 is
    used, eval.py:162-166) or None; gt_alpha [H,W] (batch['alpha'][:,:,0]) or None (IoU nan); bgcolor: cfg.bgcolor / 255.
    Both 8-bit images are built by assemble_uint8_device; only the record crosses PCIe.
    -> dict of the seven per-frame numbers (KEYS) as Python floats; with_images=True: (dict, {'rgb', 'truth', 'alpha'}
    uint8 [H,W,3] GPU images: the panels of eval.py's output)."""
    from .image import assemble_uint8_device
    rgb_img, alpha_img = assemble_uint8_device(width, height, ray_index, bgcolor, rgb, alpha, want_alpha=with_images)
    truth_img, _ = assemble_uint8_device(width, height, ray_index, bgcolor, target_rgb, None, want_alpha=False)
    alpha_map = pixel_map(ray_index, alpha.reshape(-1), height, width, torch.float32)
    body = pixel_map(ray_index, torch.ones_like(ray_index, dtype=torch.uint8), height, width, torch.uint8)
    gt_vis = None
    if ray_alpha is not None:
        ra = ray_alpha if ray_alpha.dim() == 1 else ray_alpha[:, 0]
        gt_vis = pixel_map(ray_index, ra, height, width, torch.float32)
    gt = None if gt_alpha is None else gt_alpha.to(torch.float32).contiguous()
    record, _ = _frame_metrics_raw(rgb_img, truth_img, alpha_map, body, gt_vis, gt, data_range)
    vals = record[0, :len(KEYS)].cpu().numpy()
    out = {k: float(v) for k, v in zip(KEYS, vals)}
    if with_images:
        return out, {'rgb': rgb_img, 'truth': truth_img, 'alpha': alpha_img}
    return out


def frame_metrics_from_maps(rgb, alpha, ray_index, maps, width, height, bgcolor=(1., 1., 1.), with_images=False,
                            data_range=2.0):
    """frame_metrics for a frame whose truth side is already on the device as per-pixel maps (a prepared dataset's
    device_frames, csrc/frame.hip): maps['truth_u8'] uint8 [H,W,3], maps['body'] uint8 [H,W] (the box mask),
    maps['gt_vis'] and maps['gt_alpha'] float32 [H,W].  Only the predicted image and the predicted alpha map are assembled
    here.  The same seven numbers as frame_metrics(..., target_rgbs, ray_alpha=..., gt_alpha=...) on the host dict of the
    frame, bit for bit: the kernel is handed the same bytes."""
    from .image import assemble_uint8_device
    shape = (int(height), int(width))
    for k, dtype, tail in (('truth_u8', torch.uint8, (3,)), ('body', torch.uint8, ()), ('gt_vis', torch.float32, ()),
                           ('gt_alpha', torch.float32, ())):
        if k not in maps or tuple(maps[k].shape) != shape + tail or maps[k].dtype != dtype:
            raise ValueError(f'frame_metrics_from_maps: maps[{k!r}] must be {dtype} {list(shape + tail)}')
    rgb_img, alpha_img = assemble_uint8_device(width, height, ray_index, bgcolor, rgb, alpha, want_alpha=with_images)
    alpha_map = pixel_map(ray_index, alpha.reshape(-1), height, width, torch.float32)
    record, _ = _frame_metrics_raw(rgb_img, maps['truth_u8'], alpha_map, maps['body'], maps['gt_vis'], maps['gt_alpha'],
                                   data_range)
    vals = record[0, :len(KEYS)].cpu().numpy()
    out = {k: float(v) for k, v in zip(KEYS, vals)}
    if with_images:
        return out, {'rgb': rgb_img, 'truth': maps['truth_u8'], 'alpha': alpha_img}
    return out


def batch_metrics(pred, truth, alpha=None, body=None, gt_vis=None, gt_alpha=None, data_range=2.0, want_map=False):
    """N same-size frames in one launch pair: pred, truth uint8 [N,H,W,3]; the maps [N,H,W] as occnerf_frame_metrics takes
    them (include/occnerf_hip.h).  -> (record float64 [N, 14] on the GPU: KEYS, then n_vis, n_body, intersection, union
    and the squared-error sums over vis, body, full in 8-bit units; S map [N,H,W,3] or None)."""
    return _frame_metrics_raw(pred, truth, alpha, body, gt_vis, gt_alpha, data_range, want_map)


def record_dict(record_row):
    """One row of a record (any array-like) -> {key: float} of the seven per-frame numbers."""
    row = np.asarray(record_row, dtype=np.float64)
    return {k: float(v) for k, v in zip(KEYS, row[:len(KEYS)])}
