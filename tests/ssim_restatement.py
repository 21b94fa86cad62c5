"""Float64 restatements of the reference's eval.py per-frame metrics (eval.py:100-218), the truth the HIP kernel
(occnerf_amd/csrc/metrics.hip) is tested against.

skimage is not available, so SSIM is restated from skimage's source (skimage/metrics/_structural_similarity.py, the
releases that still accept `multichannel`) for float64 input with the defaults eval.py gets: win_size 7, uniform filter
(scipy.ndimage.uniform_filter, mode 'reflect'), use_sample_covariance=True (cov_norm 49/48), K1 = 0.01, K2 = 0.03 and
data_range = 2 (float64's dtype range is (-1, 1)).  Two independent forms:
  (a) `ssim_a`: scipy.ndimage.uniform_filter exactly as skimage calls it;
  (b) `ssim_b`: a brute-force 7x7 window over np.pad(mode='symmetric') (scipy's 'reflect' is numpy's 'symmetric').
"""
import numpy as np

K1, K2, WIN = 0.01, 0.03, 7


def _ssim_from_moments(ux, uy, uxx, uyy, uxy, data_range):
    cov_norm = WIN * WIN / (WIN * WIN - 1.0)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    C1 = (K1 * data_range) ** 2
    C2 = (K2 * data_range) ** 2
    A1, A2, B1, B2 = (2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2)
    return (A1 * A2) / (B1 * B2)


def _channel_a(X, Y, data_range):
    from scipy.ndimage import uniform_filter
    f = lambda im: uniform_filter(im, size=WIN)          # noqa: E731  skimage: filter_func(X, **{'size': win_size})
    return _ssim_from_moments(f(X), f(Y), f(X * X), f(Y * Y), f(X * Y), data_range)


def _channel_b(X, Y, data_range):
    p = WIN // 2

    def f(im):
        win = np.lib.stride_tricks.sliding_window_view(np.pad(im, p, mode='symmetric'), (WIN, WIN))
        return win.sum(axis=(-1, -2)) / (WIN * WIN)
    return _ssim_from_moments(f(X), f(Y), f(X * X), f(Y * Y), f(X * Y), data_range)


def _multichannel(channel_fn, im1, im2, data_range):
    X = np.asarray(im1, dtype=np.float64)
    Y = np.asarray(im2, dtype=np.float64)
    assert X.shape == Y.shape and X.ndim == 3 and min(X.shape[:2]) >= WIN
    pad = (WIN - 1) // 2
    maps = [channel_fn(X[..., c], Y[..., c], data_range) for c in range(X.shape[2])]
    mssim = np.mean([S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean(dtype=np.float64) for S in maps])
    return float(mssim), np.stack(maps, axis=-1)


def ssim_a(im1, im2, data_range=2.0):
    """structural_similarity(im1, im2, multichannel=True, full=True) -> (mssim, S[H,W,C])."""
    return _multichannel(_channel_a, im1, im2, data_range)


def ssim_b(im1, im2, data_range=2.0):
    return _multichannel(_channel_b, im1, im2, data_range)


def psnr_metric(img_pred, img_gt):
    """eval.py:77-91."""
    with np.errstate(divide='ignore', invalid='ignore'):
        mse = np.mean((img_pred - img_gt) ** 2)
        psnr = -10 * np.log(mse) / np.log(10)
    return psnr.item()


def frame_metrics(rgb_img, truth_img, alpha_map, ray_mask, gt_vis_map=None, gt_alpha=None, data_range=2.0):
    """eval.py:140-196 on host arrays: rgb_img, truth_img uint8 [H,W,3]; alpha_map float32 [H,W] (0 where no ray);
    ray_mask bool [H*W]; gt_vis_map float32 [H,W] (ray_alpha scattered by ray_mask) or None; gt_alpha float32 [H,W]
    (batch['alpha'][:,:,0]) or None.  -> dict of the seven numbers eval.py prints, plus the S map."""
    import warnings
    height, width = rgb_img.shape[:2]
    body_mask = np.zeros((height * width, 3), dtype='float32')
    body_mask[np.asarray(ray_mask).reshape(-1)] = 1.
    body_mask = body_mask.astype(bool)
    alpha_map = np.asarray(alpha_map, dtype=np.float32)
    alpha_mask = alpha_map.reshape([width * height, ]) > np.float32(0.001)
    pred_alpha_mask = alpha_map.reshape([width * height, ]) > np.float32(0.1)
    if gt_vis_map is not None:
        alpha_mask = np.asarray(gt_vis_map, dtype=np.float32).reshape(-1) > np.float32(0.5)
    iou = float('nan')
    with warnings.catch_warnings(), np.errstate(divide='ignore', invalid='ignore'):
        warnings.simplefilter('ignore', RuntimeWarning)
        if gt_alpha is not None:
            comp_mask = pred_alpha_mask.reshape([height, width])
            comp_pred = np.asarray(gt_alpha, dtype=np.float32) > np.float32(0.5)
            intersection = (comp_pred & comp_mask).sum()
            union = (comp_pred | comp_mask).sum()
            iou = float((intersection + 0.) / (union + 0.))
        rgb_n = rgb_img / 255.
        truth_n = truth_img / 255.
        flat_r, flat_t = rgb_n.reshape([width * height, 3]), truth_n.reshape([width * height, 3])
        body_psnr = psnr_metric(flat_r[body_mask], flat_t[body_mask])
        vis_psnr = psnr_metric(flat_r[alpha_mask], flat_t[alpha_mask])
        psnr = psnr_metric(rgb_n, truth_n)
        ssim, full_ssim = ssim_a(rgb_n, truth_n, data_range)
        full = full_ssim.reshape([width * height, 3])
        body_ssim = float(np.mean(full[body_mask]))
        vis_ssim = float(np.mean(full[alpha_mask]))
    return {'psnr_vis': vis_psnr, 'ssim_vis': vis_ssim, 'psnr_body': body_psnr, 'ssim_body': body_ssim,
            'psnr_full': psnr, 'ssim_full': ssim, 'iou': iou, 'S': full_ssim}
