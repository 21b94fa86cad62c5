"""GPU: the whole-frame builder (occnerf_amd/csrc/frame.hip, ops.whole_frame), the loader around it
(WholeFrames.device_frames), metrics.frame_metrics_from_maps, and eval.py / run.py on a prepared dataset.

The builder does the host path's operations on the same bytes -- integer compaction, the float64 blend with one rounding
per operator, float32 quantisation -- so everything it writes must be EQUAL to PreparedDataset.whole_frame() and to
tests/whole_frame_restatement.py: ray_index, target_rgbs, ray_alpha, truth_u8, gt_vis, gt_alpha.  rays / near / far must
equal rays8[box] of what ops.gen_rays returns for the frame; how close gen_rays is to numpy is tests/test_f_image_rays.py's
business.  Where the device loader is compared with the host loader every key must be equal, the rays included: the
dataset's cameras are float64 and gen_rays then performs numpy's operations in numpy's order."""
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import whole_frame_cases as cases
from tests import whole_frame_restatement as wfr
from tests.gpu_util import DEV, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml')


@pytest.fixture(scope='module')
def paths(tmp_path_factory):
    return cases.make_datasets(tmp_path_factory.mktemp('whole_frame'))


def gen(ds, frame):
    from occnerf_amd import ops
    f = ds.frames[frame]
    return ops.gen_rays(f['K'], f['E'], ds.height, ds.width, f['dst_bbox_min'], f['dst_bbox_max'], DEV)


def to_numpy(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def compare_rows(got, rays8, box):
    """The ray rows of a builder result against the compaction of rays8 by `box` (a bool array) in np.nonzero's order."""
    compact = rays8[box]
    same(got['ray_index'], np.nonzero(box)[0].astype(np.int64), 'ray_index')
    same(got['rays'][0], compact[:, 0:3], 'rays_o')
    same(got['rays'][1], compact[:, 3:6], 'rays_d')
    same(got['near'], compact[:, 6:7], 'near')
    same(got['far'], compact[:, 7:8], 'far')


@pytest.mark.parametrize('bg', list(cases.BGCOLORS))
@pytest.mark.parametrize('name', list(cases.CASES))
def test_builder_equals_the_host_frame(name, bg, paths):
    from occnerf_amd import ops
    bgcolor = cases.BGCOLORS[bg]
    ds, frame = cases.open_case(name, paths, device=DEV)
    w = ds.whole_frame(frame, bgcolor)
    print('\n   ' + cases.check_condition(name, ds, frame, w))
    rays8, box = gen(ds, frame)
    box_np = box.cpu().numpy().astype(bool)
    same(box_np, w['ray_mask'], 'box mask (gen_rays) vs the host ray_mask')
    got = to_numpy(ops.whole_frame(ds._dev['image'][frame], ds._dev['alpha'][frame], rays8, box, bgcolor))
    R = int(w['ray_mask'].sum())
    assert got['ray_index'].shape == (R,) and got['rays'].shape == (2, R, 3) and got['ray_alpha'].dtype == np.float64
    compare_rows(got, rays8.cpu().numpy(), box_np)
    same(got['target_rgbs'], w['target_rgbs'], 'target_rgbs')
    same(got['ray_alpha'], w['ray_alpha'], 'ray_alpha')
    truth, gt_vis, gt_alpha = wfr.maps(w, ds.alphas[frame], bgcolor)
    same(got['truth_u8'], truth, 'truth_u8')
    same(got['gt_vis'], gt_vis, 'gt_vis')
    same(got['gt_alpha'], gt_alpha, 'gt_alpha')


@pytest.mark.parametrize('kind', ['zeros', 'ones', 'bernoulli'])
def test_builder_on_arbitrary_masks(kind, paths):
    """The builder fed directly at 300 x 37 with a mask that is no box: R = 0, every pixel, and a seeded Bernoulli(0.5) mask
    whose rows compact in np.nonzero's order."""
    from occnerf_amd import ops
    ds, frame = cases.open_case('two_chunks', paths, device=DEV)
    H, W = ds.height, ds.width
    assert (H, W) == (37, 300)
    rays8, _ = gen(ds, frame)
    box_np = {'zeros': np.zeros(H * W, bool), 'ones': np.ones(H * W, bool),
              'bernoulli': np.random.RandomState(7).rand(H * W) < 0.5}[kind]
    box = torch.from_numpy(box_np.astype(np.uint8)).to(DEV)
    bgcolor = cases.BGCOLORS['colour']
    got = to_numpy(ops.whole_frame(ds._dev['image'][frame], ds._dev['alpha'][frame], rays8, box, bgcolor))
    R = int(box_np.sum())
    assert got['ray_index'].shape == (R,) and got['rays'].shape == (2, R, 3) and got['near'].shape == (R, 1)
    assert (kind == 'zeros') == (R == 0) and (kind == 'ones') == (R == H * W)
    compare_rows(got, rays8.cpu().numpy(), box_np)
    # the host path with this mask in the place of its box test
    bg = np.array(bgcolor, dtype='float32')
    alpha = ds.alphas[frame] / 255.
    img = ((alpha * ds.images[frame] + (1.0 - alpha) * bg[None, None, :]) / 255.).astype('float32')
    w = {'img_height': H, 'img_width': W, 'ray_mask': box_np, 'target_rgbs': img.reshape(-1, 3)[box_np],
         'ray_alpha': alpha.reshape(-1, 3)[box_np]}
    same(got['target_rgbs'], w['target_rgbs'], 'target_rgbs')
    same(got['ray_alpha'], w['ray_alpha'], 'ray_alpha')
    truth, gt_vis, gt_alpha = wfr.maps(w, ds.alphas[frame], bgcolor)
    same(got['truth_u8'], truth, 'truth_u8')
    same(got['gt_vis'], gt_vis, 'gt_vis')
    same(got['gt_alpha'], gt_alpha, 'gt_alpha')
    if kind == 'zeros':                                        # maps all background
        bg8 = (255. * (bg.astype(np.float64) / 255.).astype('float32')).astype(np.uint8)
        assert (got['truth_u8'] == bg8).all() and (got['gt_vis'] == 0).all()


def test_whole_frame_refuses_bad_arguments(paths):
    from occnerf_amd import ops
    ds, frame = cases.open_case('wide', paths, device=DEV)
    img, alpha = ds._dev['image'][frame], ds._dev['alpha'][frame]
    H, W = ds.height, ds.width
    rays8, box = gen(ds, frame)
    bg = [255., 255., 255.]
    with pytest.raises(RuntimeError, match='image must be a CUDA'):
        ops.whole_frame(img.cpu(), alpha, rays8, box, bg)
    with pytest.raises(RuntimeError, match='alpha must be torch.uint8'):
        ops.whole_frame(img, alpha.float(), rays8, box, bg)
    with pytest.raises(RuntimeError, match='box_mask must be torch.uint8'):
        ops.whole_frame(img, alpha, rays8, box.bool(), bg)
    with pytest.raises(RuntimeError, match='rays8 must be a contiguous'):
        ops.whole_frame(img, alpha, torch.empty(8, H * W, device=DEV).t(), box, bg)
    big = torch.empty(1 << 14, 1 << 14, 3, device=DEV, dtype=torch.uint8)          # H * W = 2^28, never touched
    with pytest.raises(RuntimeError, match='below 2\\^28'):
        ops.whole_frame(big, big, rays8, box, bg)
    del big
    row_start = ops.whole_frame_count(box, H, W)
    R = int(row_start[H].item())
    assert R == int(box.sum().item())
    with pytest.raises(RuntimeError, match=r"out\['ray_index'\] must be"):
        ops.whole_frame(img, alpha, rays8, box, bg, row_start=row_start, R=R - 1, out=ops.alloc_whole_frame(H, W, R, DEV))
    with pytest.raises(RuntimeError, match='outside'):
        ops.whole_frame(img, alpha, rays8, box, bg, row_start=row_start, R=H * W + 1)
    with pytest.raises(RuntimeError, match='come together'):
        ops.whole_frame(img, alpha, rays8, box, bg, R=R)
    torch.cuda.synchronize()


def _frames(loader, prefetch):
    out = []
    for data, key, meta in loader.device_frames(DEV, prefetch=prefetch, data_type='movement'):
        torch.cuda.synchronize()
        out.append(({k: v.cpu().numpy().copy() for k, v in data.items()}, key,
                    {k: (v.cpu().numpy().copy() if torch.is_tensor(v) else v) for k, v in meta.items()}))
    return out


def test_device_frames_prefetch_equals_inline_equals_the_host_loader(tmp_path, monkeypatch):
    from occnerf_amd import config, sequence
    from occnerf_amd.dataset import PreparedDataset, WholeFrames
    path = str(tmp_path / 'three')
    cases.load_tool().make_dataset(path, frames=3, width=64, height=64, seed=21, focal=900.0)
    bgcolor = [30., 200., 90.]
    loader = WholeFrames(PreparedDataset(path, device=None, volume_size=4), bgcolor)
    a, b = _frames(loader, True), _frames(loader, False)
    assert len(a) == len(b) == 3
    for (da, ka, ma), (db, kb, mb) in zip(a, b):
        assert ka == kb and sorted(da) == sorted(db) and sorted(ma) == sorted(mb)
        for k in da:
            same(da[k], db[k], f'prefetch vs inline data[{k}]')
        for k in ma:
            same(ma[k], mb[k], f'prefetch vs inline meta[{k}]')
    # the host loader through today's frames_to_device (`device_frames False`), on the GPU
    cfg = config.default_cfg()
    cfg.device_frames = False
    monkeypatch.setattr(sequence, 'get_cfg', lambda: cfg)
    host = list(sequence.frames_to_device(loader, 'movement', DEV))
    torch.cuda.synchronize()
    assert len(host) == 3
    for i, ((dh, kh, mh), (da, ka, ma)) in enumerate(zip(host, a)):
        assert kh == ka and sorted(dh) == sorted(da), (kh, ka, sorted(dh), sorted(da))
        for k in dh:
            h = dh[k].cpu().numpy()
            assert h.dtype == da[k].dtype, k
            if k in ('rays', 'near', 'far'):                   # gen_rays against numpy's rays: printed before it is asserted
                print(f'   frame {i} {k}: max |device - host| = {float(np.abs(h - da[k]).max()):.3e}')
            same(da[k], h, f'device vs host data[{k}]')
        for k in mh:
            same(ma[k], mh[k].cpu().numpy() if torch.is_tensor(mh[k]) else mh[k], f'device vs host meta[{k}]')
        w = loader.dataset.whole_frame(i, bgcolor)
        assert ma['frame_name'] == w['frame_name'] and ma['target_rgbs'] is not None
        truth, gt_vis, gt_alpha = wfr.maps(w, loader.dataset.alphas[i], bgcolor)
        same(ma['truth_u8'], truth, 'truth_u8')
        same(ma['gt_vis'], gt_vis, 'gt_vis')
        same(ma['gt_alpha'], gt_alpha, 'gt_alpha')
        same(ma['body'].astype(bool), w['ray_mask'].reshape(64, 64), 'body')
        same(ma['target_rgbs'], w['target_rgbs'], 'meta target_rgbs')
        same(ma['ray_alpha'], w['ray_alpha'], 'meta ray_alpha')


def test_device_frames_names_the_frame_whose_box_misses_the_image(tmp_path):
    from occnerf_amd.dataset import PreparedDataset, WholeFrames
    path = str(tmp_path / 'miss')
    cases.load_tool().make_dataset(path, frames=2, width=48, height=40, seed=3, focal=900.0)
    with open(os.path.join(path, 'cameras.pkl'), 'rb') as f:
        cams = pickle.load(f)
    cams['frame_000001']['intrinsics'] = np.array(cams['frame_000001']['intrinsics']).copy()
    cams['frame_000001']['intrinsics'][0, 2] += 1e5
    with open(os.path.join(path, 'cameras.pkl'), 'wb') as f:
        pickle.dump(cams, f)
    ds = PreparedDataset(path, device=None, volume_size=4)
    assert ds.whole_frame(1, [0., 0., 0.])['ray_mask'].sum() == 0 and ds.whole_frame(0, [0., 0., 0.])['ray_mask'].sum() > 0
    for prefetch in (True, False):
        it = WholeFrames(ds, [0., 0., 0.]).device_frames(DEV, prefetch=prefetch)
        assert next(it)[2]['frame_name'] == 'frame_000000'
        with pytest.raises(ValueError, match='frame_000001'):
            next(it)
    torch.cuda.synchronize()


@pytest.mark.parametrize('name', ['wide', 'tiny'])
def test_frame_metrics_from_maps_equals_frame_metrics(name, paths):
    from occnerf_amd import metrics, ops
    bgcolor = cases.BGCOLORS['white']
    ds, frame = cases.open_case(name, paths, device=DEV)
    w = ds.whole_frame(frame, bgcolor)
    cases.check_condition(name, ds, frame, w)
    H, W = ds.height, ds.width
    rays8, box = gen(ds, frame)
    same(box.cpu().numpy().astype(bool), w['ray_mask'], 'box mask vs the host ray_mask')
    out = ops.whole_frame(ds._dev['image'][frame], ds._dev['alpha'][frame], rays8, box, bgcolor)
    R = int(w['ray_mask'].sum())
    g = torch.Generator().manual_seed(5)
    rgb, alpha = torch.rand(R, 3, generator=g).to(DEV), torch.rand(R, generator=g).to(DEV)
    bg01 = np.array(bgcolor) / 255.
    maps = dict(out, body=box.view(H, W))
    got, imgs = metrics.frame_metrics_from_maps(rgb, alpha, out['ray_index'], maps, W, H, bgcolor=bg01, with_images=True)
    ray_index = torch.from_numpy(np.nonzero(w['ray_mask'])[0]).to(DEV)
    _, _, gt_alpha = wfr.maps(w, ds.alphas[frame], bgcolor)
    want, wimgs = metrics.frame_metrics(rgb, alpha, ray_index, torch.from_numpy(w['target_rgbs']).to(DEV), W, H,
                                        ray_alpha=torch.from_numpy(w['ray_alpha']).to(DEV),
                                        gt_alpha=torch.from_numpy(gt_alpha).to(DEV), bgcolor=bg01, with_images=True)
    print(f'\n   {name}: ' + ', '.join(f'{k} {got[k]!r}' for k in metrics.KEYS))
    for k in metrics.KEYS:
        assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), (k, got[k], want[k])
    assert name != 'wide' or all(np.isfinite(got[k]) for k in metrics.KEYS)
    for k in ('rgb', 'truth', 'alpha'):
        assert torch.equal(imgs[k], wimgs[k]), k


def _make_eval_dataset(tmp_path, frames, width, height):
    path = str(tmp_path / 'data')
    cases.load_tool().make_dataset(path, frames=frames, width=width, height=height, seed=31, focal=900.0)
    return path


def test_eval_py_on_a_prepared_dataset(tmp_path):
    """python eval.py on a tool-made dataset: three frame lines in the reference's format, metrics.json with the dataset
    as its source, no teacher network, panels named by the frames, and the middle third of the first panel is the host
    path's truth image byte for byte."""
    from PIL import Image
    from occnerf_amd.dataset import PreparedDataset
    path = _make_eval_dataset(tmp_path, 3, 64, 64)
    cmd = [sys.executable, os.path.join(ROOT, 'eval.py'), '--cfg', CFG, 'train.dataset_path', path, 'resize_img_scale', '1.0',
           'N_samples', '32', 'load_net', 'seeded']
    out = subprocess.run(cmd, cwd=str(tmp_path), env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True,
                         timeout=170)
    assert out.returncode == 0, out.stderr[-3000:]
    num = r'(-?[0-9.]+|nan|inf)'
    frame_re = re.compile(rf'^PSNR-vis: {num}, SSIM-vis: {num}; PSNR-body: {num}, SSIM-body: {num}; PSNR-full: {num}, '
                          rf'SSIM-full: {num}, IOU: {num}$')
    lines = out.stdout.splitlines()
    assert len([l for l in lines if frame_re.match(l)]) == 3, out.stdout[-3000:]
    assert 'targets are the dataset images (no teacher network)' in out.stdout
    folder = tmp_path / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'seeded' / 'eval'
    rec = json.load(open(folder / 'metrics.json'))
    assert rec['n_frames'] == 3 and rec['source'] == 'dataset'
    assert [f['frame'] for f in rec['frames']] == ['frame_000000', 'frame_000001', 'frame_000002']
    for f in rec['frames']:
        assert np.isfinite(f['psnr_full']) and np.isfinite(f['ssim_full']) and 0.0 <= f['iou'] <= 1.0, f
    ds = PreparedDataset(path, device=None)
    w = ds.whole_frame(0, [255., 255., 255.])
    truth, _, _ = wfr.maps(w, ds.alphas[0], [255., 255., 255.])
    panel = np.asarray(Image.open(folder / 'frame_000000.png'))
    assert panel.shape == (64, 192, 3)
    same(panel[:, 64:128], truth, 'the truth third of the first panel')


def test_run_py_movement_on_a_prepared_dataset(tmp_path):
    path = _make_eval_dataset(tmp_path, 2, 48, 40)
    cmd = [sys.executable, os.path.join(ROOT, 'run.py'), '--cfg', CFG, '--type', 'movement', 'train.dataset_path', path,
           'resize_img_scale', '1.0', 'N_samples', '32', 'load_net', 'seeded']
    out = subprocess.run(cmd, cwd=str(tmp_path), env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True,
                         timeout=170)
    assert out.returncode == 0, out.stderr[-3000:]
    folder = tmp_path / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'seeded' / 'movement'
    assert sorted(os.listdir(folder)) == ['000000.png', '000001.png']
    assert re.search(r'^\d+ rays in [0-9.]+ s -> \d+ rays/s', out.stdout, flags=re.M), out.stdout[-2000:]
