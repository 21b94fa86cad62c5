"""eval.py's per-frame metrics (occnerf_amd/metrics.py, csrc/metrics.hip) and the eval.py entry point.

The truth is tests/ssim_restatement.py: skimage's SSIM restated from its source in float64 (skimage is not available), in
two independent forms that are pinned to each other on the CPU; the HIP kernel is compared with form (a)."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ssim_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
C1, C2 = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2


# ------------------------------------------------------------------------------------------------ CPU: the restatement

@pytest.mark.parametrize('hw', [(7, 7), (9, 13), (33, 20), (64, 64)])
def test_two_restatements_agree(hw):
    rng = np.random.default_rng(hw[0] * 100 + hw[1])
    x = rng.integers(0, 256, size=hw + (3,), dtype=np.uint8) / 255.
    y = rng.integers(0, 256, size=hw + (3,), dtype=np.uint8) / 255.
    ma, Sa = R.ssim_a(x, y)
    mb, Sb = R.ssim_b(x, y)
    assert Sa.shape == hw + (3,)
    assert np.abs(Sa - Sb).max() <= 1e-12
    assert abs(ma - mb) <= 1e-12
    # related but not identical images: structure in S, not a constant
    z = np.clip(x + rng.integers(-8, 9, size=x.shape) / 255., 0, 1)
    assert np.abs(R.ssim_a(x, z)[1] - R.ssim_b(x, z)[1]).max() <= 1e-12


@pytest.mark.parametrize('a,b', [(0, 0), (0, 255), (17, 200), (255, 254), (128, 128)])
def test_constant_images_closed_form(a, b):
    x = np.full((11, 9, 3), a / 255.)
    y = np.full((11, 9, 3), b / 255.)
    fa, fb = a / 255., b / 255.
    want = (2 * fa * fb + C1) / (fa * fa + fb * fb + C1)
    for fn in (R.ssim_a, R.ssim_b):
        m, S = fn(x, y)
        assert np.abs(S - want).max() <= 1e-12 and abs(m - want) <= 1e-12


def test_binding_covers_the_metrics_entries_and_refuses_bad_arguments():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from occnerf_amd import _lib, metrics
    header = open(os.path.join(ROOT, 'include', 'occnerf_hip.h')).read()
    for name in ('occnerf_frame_metrics_workspace_bytes', 'occnerf_frame_metrics'):
        assert name in _lib.SIGNATURES and re.search(rf'\b{name}\s*\(', header)
    assert re.search(rf'#define OCCNERF_FRAME_METRICS_RECORD {metrics.RECORD}\b', header)
    lib = _lib.lib()
    assert lib.occnerf_abi_version() == 5
    assert lib.occnerf_frame_metrics_workspace_bytes(2, 512, 512) == 2 * 8 * 32 * 80
    assert lib.occnerf_frame_metrics_workspace_bytes(1, 7, 7) == 80
    for n, h, w in ((0, 16, 16), (1, 6, 16), (1, 16, 6)):
        assert lib.occnerf_frame_metrics_workspace_bytes(n, h, w) == -1
    rc = lib.occnerf_frame_metrics(None, None, None, None, None, None, 1, 16, 16, 2.0, None, None, None, None)
    assert rc != 0 and b'null' in lib.occnerf_last_error()
    # non-null (host) pointers that are never dereferenced: the sizes are refused before any launch
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    rc = lib.occnerf_frame_metrics(p, p, None, None, None, None, 1, 6, 16, 2.0, p, None, p, None)
    assert rc != 0 and b'bad sizes' in lib.occnerf_last_error()
    rc = lib.occnerf_frame_metrics(p, p, None, None, None, None, 1, 16, 16, 0.0, p, None, p, None)
    assert rc != 0 and b'data_range' in lib.occnerf_last_error()


def test_structural_similarity_refuses_what_is_not_built():
    from occnerf_amd.metrics import structural_similarity
    for kw, word in (({'gradient': True}, 'gradient'), ({'gaussian_weights': True}, 'gaussian_weights'),
                     ({'win_size': 11}, 'win_size'), ({'use_sample_covariance': False}, 'use_sample_covariance'),
                     ({'K1': 0.02}, 'K1'), ({'sigma': 1.5}, 'sigma'), ({'multichannel': False}, 'multichannel')):
        with pytest.raises(NotImplementedError, match=word):
            structural_similarity(None, None, **kw)


# ------------------------------------------------------------------------------------------------ GPU: kernel vs (a)

def _close(got, want, rel=None, abs_=None):
    if math.isnan(want):
        return math.isnan(got)
    if math.isinf(want):
        return got == want
    if rel is not None:
        return abs(got - want) <= rel * abs(want)
    return abs(got - want) <= abs_


def _random_masks(rng, H, W):
    alpha = rng.uniform(0, 1, size=(H, W)).astype(np.float32)
    alpha[rng.uniform(size=(H, W)) < 0.3] = 0.0
    alpha[rng.uniform(size=(H, W)) < 0.05] = np.float32(0.001)
    alpha[rng.uniform(size=(H, W)) < 0.05] = np.float32(0.1)
    body = alpha > 0
    body |= rng.uniform(size=(H, W)) < 0.1
    alpha[~body] = 0.0
    gt_alpha = (rng.uniform(size=(H, W)) < 0.5).astype(np.float32)
    gt_alpha[rng.uniform(size=(H, W)) < 0.05] = np.float32(0.5)
    return alpha, body, gt_alpha


def _gpu(pred, truth, alpha=None, body=None, gt_vis=None, gt_alpha=None):
    """One frame through the kernel -> (record [14] numpy, S map [H,W,3] numpy)."""
    from occnerf_amd import metrics
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(DEV)  # noqa: E731
    rec, smap = metrics.batch_metrics(t(pred, np.uint8)[None], t(truth, np.uint8)[None],
                                      None if alpha is None else t(alpha, np.float32)[None],
                                      None if body is None else t(body, np.uint8)[None],
                                      None if gt_vis is None else t(gt_vis, np.float32)[None],
                                      None if gt_alpha is None else t(gt_alpha, np.float32)[None], want_map=True)
    return rec[0].cpu().numpy(), smap[0].cpu().numpy()


def _check_against_restatement(pred, truth, alpha, body, gt_vis=None, gt_alpha=None):
    from occnerf_amd.metrics import record_dict
    rec, S = _gpu(pred, truth, alpha, body, gt_vis, gt_alpha)
    want = R.frame_metrics(pred, truth, alpha, body.reshape(-1), gt_vis, gt_alpha)
    assert np.abs(S - want['S']).max() <= 1e-10
    got = record_dict(rec)
    for k in ('ssim_full', 'ssim_body', 'ssim_vis'):
        assert _close(got[k], want[k], abs_=1e-11), (k, got[k], want[k])
    for k in ('psnr_full', 'psnr_body', 'psnr_vis'):
        assert _close(got[k], want[k], rel=1e-12), (k, got[k], want[k])
    assert _close(got['iou'], want['iou'], rel=0.0), (got['iou'], want['iou'])
    return rec, S, want


@pytest.mark.gpu
@pytest.mark.parametrize('hw', [(512, 512), (7, 7), (31, 517), (17, 65), (23, 130), (65, 63), (8, 200)])
def test_kernel_matches_restatement_on_random_frames(hw):
    rng = np.random.default_rng(hw[0] * 1000 + hw[1])
    H, W = hw
    pred = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    truth = np.clip(pred.astype(int) + rng.integers(-40, 41, size=pred.shape), 0, 255).astype(np.uint8)
    truth[rng.uniform(size=(H, W)) < 0.2] = rng.integers(0, 256, size=3, dtype=np.uint8)
    alpha, body, gt_alpha = _random_masks(rng, H, W)
    rec, _, _ = _check_against_restatement(pred, truth, alpha, body, None, gt_alpha)
    assert rec[8] == body.sum() and rec[7] == (alpha > np.float32(0.001)).sum()


@pytest.mark.gpu
def test_mostly_white_frame_with_a_small_body():
    rng = np.random.default_rng(5)
    H, W = 128, 96
    pred = np.full((H, W, 3), 255, np.uint8)
    truth = pred.copy()
    alpha = np.zeros((H, W), np.float32)
    body = np.zeros((H, W), bool)
    body[50:62, 40:49] = True
    pred[body] = rng.integers(0, 256, size=(body.sum(), 3), dtype=np.uint8)
    truth[body] = np.clip(pred[body].astype(int) + rng.integers(-20, 21, size=(body.sum(), 3)), 0, 255)
    alpha[body] = rng.uniform(0, 1, size=body.sum()).astype(np.float32)
    gt_alpha = np.zeros((H, W), np.float32)
    gt_alpha[52:64, 41:50] = 1.0
    rec, S, want = _check_against_restatement(pred, truth, alpha, body, None, gt_alpha)
    assert S[0, 0, 0] == 1.0 and 0 < want['ssim_body'] < 1


@pytest.mark.gpu
def test_identical_images_give_exactly_one_and_infinite_psnr():
    rng = np.random.default_rng(7)
    pred = rng.integers(0, 256, size=(37, 70, 3), dtype=np.uint8)
    alpha, body, gt_alpha = _random_masks(rng, 37, 70)
    rec, S = _gpu(pred, pred, alpha, body, None, gt_alpha)
    assert np.all(S == 1.0)
    assert rec[1] == 1.0 and rec[3] == 1.0 and rec[5] == 1.0
    assert rec[0] == np.inf and rec[2] == np.inf and rec[4] == np.inf
    from occnerf_amd.metrics import structural_similarity
    t = torch.from_numpy(pred).to(DEV)
    m, Smap = structural_similarity(t, t.clone(), full=True)
    assert m == 1.0 and bool((Smap == 1.0).all())


@pytest.mark.gpu
def test_vis_and_iou_masks_use_float32_thresholds():
    H, W = 16, 16
    rng = np.random.default_rng(11)
    pred = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    truth = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    alpha = np.zeros((H, W), np.float32)
    t1, t2 = np.float32(0.001), np.float32(0.1)
    alpha[:4] = t1                                             # not in vis
    alpha[4:8] = np.nextafter(t1, np.float32(1))               # in vis
    alpha[8:12] = t2                                           # in vis, not in the IoU's prediction
    alpha[12:] = np.nextafter(t2, np.float32(1))               # in both
    assert float(t1) != 0.001                                  # the float32 constant is not the float64 one
    body = np.ones((H, W), bool)
    gt_alpha = np.zeros((H, W), np.float32)
    gt_alpha[:, :8] = np.float32(0.5)                          # not in
    gt_alpha[:, 8:] = np.nextafter(np.float32(0.5), np.float32(1))
    rec, _, _ = _check_against_restatement(pred, truth, alpha, body, None, gt_alpha)
    assert rec[7] == 12 * W                                    # n_vis
    assert rec[9] == 4 * 8 and rec[10] == 4 * W + 12 * 8       # intersection, union


@pytest.mark.gpu
def test_ray_alpha_vis_path_and_empty_union():
    rng = np.random.default_rng(13)
    H, W = 40, 50
    pred = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    truth = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    alpha, body, gt_alpha = _random_masks(rng, H, W)
    gt_vis = np.where(body, rng.uniform(0, 1, size=(H, W)), 0).astype(np.float32)
    gt_vis[body & (rng.uniform(size=(H, W)) < 0.1)] = np.float32(0.5)
    rec, _, want = _check_against_restatement(pred, truth, alpha, body, gt_vis, gt_alpha)
    assert rec[7] == (gt_vis > np.float32(0.5)).sum()
    # union 0 -> nan; empty vis / body -> nan; no gt alpha -> nan IoU
    rec, _, want = _check_against_restatement(pred, truth, np.zeros((H, W), np.float32), np.zeros((H, W), bool),
                                              None, np.zeros((H, W), np.float32))
    assert math.isnan(rec[6]) and math.isnan(rec[0]) and math.isnan(rec[1]) and math.isnan(rec[3])
    rec, _ = _gpu(pred, truth, alpha, body, None, None)
    assert math.isnan(rec[6])


@pytest.mark.gpu
def test_batch_equals_single_frames_and_runs_are_bitwise_identical():
    from occnerf_amd import metrics
    rng = np.random.default_rng(17)
    N, H, W = 3, 45, 77
    pred = torch.from_numpy(rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)).to(DEV)
    truth = torch.from_numpy(rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)).to(DEV)
    masks = [_random_masks(rng, H, W) for _ in range(N)]
    alpha = torch.from_numpy(np.stack([m[0] for m in masks])).to(DEV)
    body = torch.from_numpy(np.stack([m[1] for m in masks]).astype(np.uint8)).to(DEV)
    gt = torch.from_numpy(np.stack([m[2] for m in masks])).to(DEV)
    rec, S = metrics.batch_metrics(pred, truth, alpha, body, None, gt, want_map=True)
    rec2, S2 = metrics.batch_metrics(pred, truth, alpha, body, None, gt, want_map=True)
    assert torch.equal(rec, rec2) and torch.equal(S, S2)
    assert torch.equal(rec.view(torch.int64), rec2.view(torch.int64))
    for i in range(N):
        r1, s1 = metrics.batch_metrics(pred[i:i + 1], truth[i:i + 1], alpha[i:i + 1], body[i:i + 1], None, gt[i:i + 1],
                                       want_map=True)
        assert torch.equal(r1[0].view(torch.int64), rec[i].view(torch.int64)) and torch.equal(s1[0], S[i])


@pytest.mark.gpu
def test_structural_similarity_api_takes_uint8_and_exact_float_images():
    from occnerf_amd.metrics import structural_similarity
    rng = np.random.default_rng(19)
    x = rng.integers(0, 256, size=(20, 30, 3), dtype=np.uint8)
    y = rng.integers(0, 256, size=(20, 30, 3), dtype=np.uint8)
    want_m, want_S = R.ssim_a(x / 255., y / 255.)
    xt, yt = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    m = structural_similarity(xt, yt)
    assert isinstance(m, float) and abs(m - want_m) <= 1e-11
    m2, S = structural_similarity(xt.double() / 255., yt.double() / 255., full=True, multichannel=True)
    assert m2 == m and S.shape == (20, 30, 3) and np.abs(S.cpu().numpy() - want_S).max() <= 1e-10
    m3 = structural_similarity(xt, yt, data_range=1.0)
    assert abs(m3 - R.ssim_a(x / 255., y / 255., data_range=1.0)[0]) <= 1e-11
    with pytest.raises(ValueError, match='1/255'):
        structural_similarity(xt.double() / 255. + 1e-6, yt.double() / 255.)


@pytest.mark.gpu
def test_rendered_frame_against_its_teacher():
    """A frame of the seeded network and of the amplified teacher (run.py `_teacher`'s checkpoint kind): frame_metrics on
    the device rays against the restatement on the host images of unpack_to_image."""
    from occnerf_amd import metrics, synth
    from occnerf_amd.image import unpack_to_image
    from occnerf_amd.seeded import build_network, frame_to_device
    H = W = 64
    frame = synth.make_frame(img_size=H, pose72=synth.movement_pose(1, 4))
    data = frame_to_device(frame, DEV)
    outs = []
    for seed, amplify in ((0, False), (1, True)):
        net = build_network(seed=seed, amplify=amplify, S=16)
        with torch.no_grad():
            outs.append(net(**data, iter_val=1e7))
    out, target = outs
    torch.cuda.synchronize()
    mask = np.asarray(frame['ray_mask']).reshape(-1).astype(bool)
    ray_index = torch.from_numpy(np.nonzero(mask)[0]).to(DEV)
    ray_alpha = (target['alpha'] / target['alpha'].max()).reshape(-1, 1)     # a gt silhouette: the teacher's, normalised
    gt_alpha_map = metrics.pixel_map(ray_index, ray_alpha[:, 0], H, W, torch.float32)
    host = lambda t: t.detach().cpu().numpy()  # noqa: E731
    rgb_img, _, truth_img = unpack_to_image(W, H, mask, np.ones(3), host(out['rgb']), host(out['alpha']),
                                            host(target['rgb']))
    alpha_map = np.zeros(H * W, np.float32)
    alpha_map[mask] = host(out['alpha']).reshape(-1)
    gt_map = np.zeros(H * W, np.float32)
    gt_map[mask] = host(ray_alpha).reshape(-1)
    for ra in (None, ray_alpha):
        got = metrics.frame_metrics(out['rgb'], out['alpha'], ray_index, target['rgb'], W, H, ray_alpha=ra,
                                    gt_alpha=gt_alpha_map)
        want = R.frame_metrics(rgb_img, truth_img, alpha_map.reshape(H, W), mask,
                               None if ra is None else gt_map.reshape(H, W), gt_map.reshape(H, W))
        for k in metrics.KEYS:
            if k.startswith('ssim'):
                assert _close(got[k], want[k], abs_=1e-11), (k, got[k], want[k])
            else:
                assert _close(got[k], want[k], rel=1e-12), (k, got[k], want[k])
        assert all(math.isfinite(got[k]) for k in metrics.KEYS), got
        assert got['ssim_full'] < 1.0 and 0.0 <= got['iou'] <= 1.0


# ------------------------------------------------------------------------------------------------ GPU: eval.py

@pytest.mark.gpu
def test_eval_py_entry_point(tmp_path):
    """eval.py on the synthetic source: the reference's per-frame and final lines with finite values; the PNG panels it
    wrote, recomputed with restatement (a), give the numbers of metrics.json, whose means are the printed ones."""
    from PIL import Image
    from occnerf_amd.rays import frame_rays
    from occnerf_amd.sequence import SyntheticFrames
    cmd = [sys.executable, os.path.join(ROOT, 'eval.py'), '--cfg', os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml'),
           'render_size', '32', 'N_samples', '16', 'render_frames', '4']
    out = subprocess.run(cmd, cwd=str(tmp_path), env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    num = r'(-?[0-9.]+|nan|inf)'
    frame_re = re.compile(rf'^PSNR-vis: {num}, SSIM-vis: {num}; PSNR-body: {num}, SSIM-body: {num}; PSNR-full: {num}, '
                          rf'SSIM-full: {num}, IOU: {num}$')
    lines = out.stdout.splitlines()
    per_frame = [frame_re.match(l) for l in lines if frame_re.match(l)]
    assert len(per_frame) == 4, out.stdout[-3000:]
    for m in per_frame:
        assert all(math.isfinite(float(v)) for v in m.groups()), m.group(0)
    iou_line = [l for l in lines if l.startswith('IOU ')]
    final = [l for l in lines if l.startswith('PSNR_vis ')]
    assert len(iou_line) == 1 and len(final) == 1
    fm = re.match(r'^PSNR_vis (\S+), SSIM_vis (\S+); PSNR_body (\S+), SSIM_body (\S+); PSNR_full (\S+), SSIM_full (\S+)$',
                  final[0])
    assert fm, final[0]
    folder = tmp_path / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'seeded' / 'eval'
    rec = json.load(open(folder / 'metrics.json'))
    assert len(rec['frames']) == 4
    mean = rec['mean']
    assert float(iou_line[0].split()[1]) == mean['iou']
    printed = [float(v) for v in fm.groups()]
    assert printed == [mean[k] for k in ('psnr_vis', 'ssim_vis', 'psnr_body', 'ssim_body', 'psnr_full', 'ssim_full')]
    for k in mean:
        assert mean[k] == float(np.mean([f[k] for f in rec['frames']]))
    for m, f in zip(per_frame, rec['frames']):                 # the printed %.4f values are the recorded ones
        assert all(abs(float(v) - f[k]) <= 5.01e-5 for v, k in zip(m.groups(), ('psnr_vis', 'ssim_vis', 'psnr_body',
                                                                                'ssim_body', 'psnr_full', 'ssim_full', 'iou')))
    # recompute full and body from the written panels; body = the frame's ray mask, as eval.py's device rays form it
    src = SyntheticFrames('movement', img_size=32, render_frames=4, device_rays=True)
    for idx, batch in enumerate(src):
        fr = frame_rays(batch['camera_K'][0].numpy(), batch['camera_E'][0].numpy(), 32, 32, batch['dst_bbox_min'][0].numpy(),
                        batch['dst_bbox_max'][0].numpy(), DEV)
        mask = fr['ray_mask'].cpu().numpy().astype(bool)
        f = rec['frames'][idx]
        panel = np.asarray(Image.open(folder / f"{f['frame']}.png"))
        assert panel.shape == (32, 96, 3)
        rgb_img, truth_img = panel[:, :32], panel[:, 32:64]
        x, y = rgb_img / 255., truth_img / 255.
        m_full, S = R.ssim_a(x, y)
        body = np.repeat(mask[:, None], 3, 1)
        assert abs(m_full - f['ssim_full']) <= 1e-9
        assert abs(float(np.mean(S.reshape(-1, 3)[body])) - f['ssim_body']) <= 1e-9
        assert abs(R.psnr_metric(x, y) - f['psnr_full']) <= 1e-9
        assert abs(R.psnr_metric(x.reshape(-1, 3)[body], y.reshape(-1, 3)[body]) - f['psnr_body']) <= 1e-9
