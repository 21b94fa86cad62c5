"""GPU: resizing dataset frames on the device (occnerf_amd/csrc/resize.hip, ops.resize_frame), the float64 pixel source of
the batch and frame builders (ops.patch_batch_f64, ops.whole_frame_f64), the loaders around them and the three entry points
on a dataset opened with `train.resize_frames True resize_img_scale 0.5`.

The kernel performs the operations of occnerf_amd/resize.py in the same order, so its result must be EQUAL to
resize_blend's; the consumers are compared with the restatements the uint8 path is held to (tests/train_batch_restatement.py,
tests/whole_frame_restatement.py), fed the frame tests/resize_cases.py restates."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from occnerf_amd import resize
from tests import resize_cases as rc
from tests import train_batch_restatement as tbr
from tests import whole_frame_restatement as wfr
from tests.gpu_util import DEV, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml')
N_PATCHES, SIZE, RATIO = 4, 16, 0.8
BG = [12.25, 200.7, 99.33]
RESIZE_OPTS = ['train.resize_frames', 'True', 'resize_img_scale', '0.5']


# ---------------------------------------------------------------- 1. the kernel is resize_blend
def device_resize(image, mask, bgcolor, s):
    from occnerf_amd import ops
    H, W = mask.shape[:2]
    tables = ops.upload_resize_tables(resize.frame_tables(H, W, s), DEV)
    img = None if image is None else torch.from_numpy(image).to(DEV)
    oi, oa = ops.resize_frame(img, torch.from_numpy(mask).to(DEV), tables, bgcolor)
    torch.cuda.synchronize()
    return (None if oi is None else oi.cpu().numpy()), oa.cpu().numpy()


@pytest.mark.parametrize('bg', list(rc.BGCOLORS))
@pytest.mark.parametrize('name', list(rc.CASES))
def test_resize_frame_equals_resize_blend(name, bg):
    H, W, s = rc.CASES[name]
    image, mask = rc.random_frame(name)
    want_img, want_alpha = resize.resize_blend(image, mask, rc.BGCOLORS[bg], s)
    got_img, got_alpha = device_resize(image, mask, rc.BGCOLORS[bg], s)
    assert got_img.dtype == got_alpha.dtype == np.float64 and got_img.shape == rc.SIZES[name] + (3,)
    same(got_alpha, want_alpha, 'alpha64')
    same(got_img, want_img, 'img64')
    assert np.array_equal(got_img, want_img) and np.array_equal(got_alpha, want_alpha)
    none, alone = device_resize(None, mask, None, s)           # the mask alone
    assert none is None
    same(alone, want_alpha, 'alpha64 without an image')


@pytest.mark.parametrize('H,W,s', [(64, 40, 0.06), (70, 33, 0.2), (12, 20, 2.0), (257, 130, 0.5)],
                         ids=['one-row-tiles', 'four-row-tiles', 'upscale', 'several-tiles-each-way'])
def test_resize_frame_at_every_tile_height(H, W, s):
    """The scales at which the entry shortens its tiles so that their source rows fit the LDS rows (1 / s > 2.3), an
    upscale, and a frame of several tiles each way whose last tiles are partial."""
    rng = np.random.RandomState(H * 1000 + W)
    image, mask = (rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2))
    want_img, want_alpha = resize.resize_blend(image, mask, BG, s)
    got_img, got_alpha = device_resize(image, mask, BG, s)
    same(got_alpha, want_alpha, 'alpha64')
    same(got_img, want_img, 'img64')


def test_resize_frame_refuses_bad_arguments():
    from occnerf_amd import ops
    tables = ops.upload_resize_tables(resize.frame_tables(40, 48, 0.5), DEV)
    image, mask = (torch.zeros(40, 48, 3, dtype=torch.uint8, device=DEV) for _ in range(2))
    with pytest.raises(RuntimeError, match='tables are those of a 48 x 40'):
        ops.resize_frame(image[:38].contiguous(), mask[:38].contiguous(), tables, BG)
    with pytest.raises(RuntimeError, match='bgcolor'):
        ops.resize_frame(image, mask, tables)
    with pytest.raises(RuntimeError, match='out must be'):
        ops.resize_frame(image, mask, tables, BG, out=ops.alloc_resize_frame(20, 25, DEV))
    with pytest.raises(RuntimeError, match='exactly when'):
        ops.resize_frame(None, mask, tables, out=ops.alloc_resize_frame(20, 24, DEV))
    with pytest.raises(RuntimeError, match='float64'):
        ops.resize_frame(None, mask, tables, out=(None, torch.zeros(20, 24, 3, device=DEV)))
    broken = dict(tables, x_lanczos=(tables['x_lanczos'][0] + 1, tables['x_lanczos'][1]))      # the host copy: column 48
    with pytest.raises(RuntimeError, match='reads outside the 48 columns'):
        ops.resize_frame(image, mask, broken, BG)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 2. the consumers of a resized frame
@pytest.fixture(scope='module')
def data_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('resize_gpu') / 'data')
    rc.load_tool().make_dataset(path, **rc.DATASET)
    return path


@pytest.fixture(scope='module')
def dataset(data_path):
    from occnerf_amd.dataset import PreparedDataset
    return PreparedDataset(data_path, device=DEV, volume_size=4, occlude=True, occlusion=rc.BAND, resize_img_scale=0.5,
                           resize_frames=True)


@pytest.fixture(scope='module')
def restated(dataset):
    """(img64, alpha64) of every frame over BG by the restatement's double loop; computed once, never written to."""
    out = [rc.restate(dataset.images[i], dataset.alphas[i], BG, 0.5) for i in range(len(dataset))]
    for pair in out:
        for a in pair:
            a.setflags(write=False)
    return out


def gen(ds, frame):
    from occnerf_amd import ops
    f = ds.frames[frame]
    return ops.gen_rays(f['K'], f['E'], ds.height, ds.width, f['dst_bbox_min'], f['dst_bbox_max'], DEV)


def resized_on_device(ds, frame, bgcolor):
    from occnerf_amd import ops
    return ops.resize_frame(ds._dev['image'][frame], ds._dev['alpha'][frame], ds._dev['resize'], bgcolor)


@pytest.mark.parametrize('frame', [0, 1, 2])
def test_whole_frame_f64_equals_the_host_rules(frame, dataset, restated):
    from occnerf_amd import ops
    ds = dataset
    assert (ds.height, ds.width, ds.src_height, ds.src_width) == (40, 48, 80, 96)
    img64, alpha64 = restated[frame]
    assert ds.frames[frame]['empty'] == (frame == 0) == bool(np.sum(alpha64) < 1)      # the band empties frame 0's resized mask
    w = rc.consumer_frame(ds, frame, BG, restated[frame])
    subject = w['ray_alpha'][:, 0] > 0
    assert (~subject).any() and subject.any() == (frame != 0)                          # both pixel classes inside the box
    host = ds.whole_frame(frame, BG)
    for k in ('ray_mask', 'target_rgbs', 'ray_alpha'):
        same(host[k], w[k], f'host whole_frame {k}')
    rays8, box = gen(ds, frame)
    box_np = box.cpu().numpy().astype(bool)
    same(box_np, w['ray_mask'], 'box mask (gen_rays) vs the host ray_mask')
    di, da = resized_on_device(ds, frame, BG)
    got = {k: v.cpu().numpy() for k, v in ops.whole_frame_f64(di, da, rays8, box, BG).items()}
    R = int(w['ray_mask'].sum())
    assert got['ray_index'].shape == (R,) and got['rays'].shape == (2, R, 3) and got['ray_alpha'].dtype == np.float64
    compact = rays8.cpu().numpy()[box_np]
    same(got['ray_index'], np.nonzero(box_np)[0].astype(np.int64), 'ray_index')
    same(got['rays'][0], compact[:, 0:3], 'rays_o')
    same(got['rays'][1], compact[:, 3:6], 'rays_d')
    same(got['near'], compact[:, 6:7], 'near')
    same(got['far'], compact[:, 7:8], 'far')
    same(got['target_rgbs'], w['target_rgbs'], 'target_rgbs')
    same(got['ray_alpha'], w['ray_alpha'], 'ray_alpha')
    truth, gt_vis, _ = wfr.maps(w, np.zeros((40, 48, 3), np.uint8), BG)
    same(got['truth_u8'], truth, 'truth_u8')
    same(got['gt_vis'], gt_vis, 'gt_vis')
    same(got['gt_alpha'], alpha64[:, :, 0].astype('float32'), 'gt_alpha')
    same(ds.gt_alpha(frame), got['gt_alpha'], 'the host gt_alpha')


def restatement_of(data_path, restated, monkeypatch):
    """tests/train_batch_restatement.py's Dataset with its load_image replaced by the restated resize (train.py:306-314 sits
    inside load_image): everything after it is the code the uint8 path is held to."""
    def load_image(dataset_path, frame_name, bg_color, idx, cfg):      # frame_masks asks with a black background: the
        assert cfg['resize_img_scale'] == 0.5                          # masks it reads do not depend on the colour
        return restated[idx]
    monkeypatch.setattr(tbr, 'load_image', load_image)
    return tbr.Restatement(data_path, N_patches=N_PATCHES, size=SIZE, sample_subject_ratio=RATIO, occlude=True, occlusion=rc.BAND,
                           volume_size=4, resize_img_scale=0.5)


@pytest.mark.parametrize('frame', [0, 1, 2])
def test_patch_batch_f64_equals_the_restatement(frame, dataset, data_path, restated, monkeypatch):
    from occnerf_amd import ops
    from tests.test_g_train_batch import compare
    ds = dataset
    rs = restatement_of(data_path, restated, monkeypatch)
    _, _, subject, off = rs.frame_masks(frame)
    u = np.array([[0.1, 0.37], [0.95, 0.81], [0.5, 0.999], [0.85, 0.02]])
    draws = tbr.draws_from_uniforms(u, subject, off, RATIO)
    print(f'\n   frame {frame}: subject {int(subject.sum())}, off-subject {int(off.sum())}, draws {draws}')
    assert off.sum() > 0 and (subject.sum() > 0) == (frame != 0)
    assert {c for c, _ in draws} == ({0, 1} if frame != 0 else {1})    # both classes drawn; an empty class falls back
    r = rs.getitem(frame, BG, draws)
    assert r['_empty'] == ds.frames[frame]['empty']
    same(ds.frames[frame]['K'], r['_K'], 'K')
    rays8, box = gen(ds, frame)
    di, da = resized_on_device(ds, frame, BG)
    out = ops.patch_batch_f64(di, da, rays8, box, N_PATCHES, SIZE, u, RATIO, BG)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    compare(got, rays8.cpu().numpy(), box.cpu().numpy().astype(bool), r, N_PATCHES, SIZE)


# ---------------------------------------------------------------- 3. the loaders
def _batches(ds, prefetch, n):
    from occnerf_amd.dataset import PatchBatchLoader
    loader = PatchBatchLoader(ds, n_patches=N_PATCHES, size=SIZE, bgcolor=None, seed=5, prefetch=prefetch)
    out = []
    for _ in range(n):
        b = next(loader)
        torch.cuda.synchronize()
        out.append({k: (v.cpu().numpy().copy() if torch.is_tensor(v) else np.copy(v)) for k, v in b.items()})
    return out


def test_loader_prefetch_equals_inline_and_equals_the_restatement(dataset, data_path, monkeypatch):
    ds = dataset
    a, b = _batches(ds, True, 5), _batches(ds, False, 5)
    assert ds.epoch_frames == [1, 2] and {int(x['frame']) for x in a} == {1, 2}
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y)
        for k in x:
            assert np.array_equal(x[k], y[k]), k
        assert x['n_rows'] == x['patch_div_indices'][-1] == x['rays'].shape[1] > 0
        assert x['target_patches'].shape == (N_PATCHES, SIZE, SIZE, 3)
    assert any(not np.array_equal(a[0]['bgcolor'], x['bgcolor']) for x in a[1:])           # a colour per batch
    # one batch against the restatement on its own draws and its own background colour
    x = a[3]
    frame = int(x['frame'])
    own = rc.restate(ds.images[frame], ds.alphas[frame], x['bgcolor'], 0.5)
    monkeypatch.setattr(tbr, 'load_image', lambda path, name, bg, idx, cfg: own)
    rs = tbr.Restatement(data_path, N_patches=N_PATCHES, size=SIZE, occlude=True, occlusion=rc.BAND, volume_size=4,
                         resize_img_scale=0.5)
    _, _, subject, off = rs.frame_masks(frame)
    r = rs.getitem(frame, x['bgcolor'], tbr.draws_from_uniforms(x['u'], subject, off, 0.8))
    same(x['target_patches'], r['target_patches'], 'loader target_patches')
    same(x['target_rgbs'], r['target_rgbs'], 'loader target_rgbs')
    same(x['patch_masks'], r['patch_masks'], 'loader patch_masks')
    same(x['patch_div_indices'], r['patch_div_indices'], 'loader patch_div_indices')


def _frames(loader, prefetch):
    out = []
    for data, key, meta in loader.device_frames(DEV, prefetch=prefetch, data_type='movement'):
        torch.cuda.synchronize()
        out.append(({k: v.cpu().numpy().copy() for k, v in data.items()}, key,
                    {k: (v.cpu().numpy().copy() if torch.is_tensor(v) else v) for k, v in meta.items()}))
    return out


def test_device_frames_prefetch_equals_inline_equals_the_host_frame(dataset):
    from occnerf_amd.dataset import WholeFrames
    loader = WholeFrames(dataset, BG)
    a, b = _frames(loader, True), _frames(loader, False)
    assert len(a) == len(b) == 3
    for i, ((da, ka, ma), (db, kb, mb)) in enumerate(zip(a, b)):
        assert ka == kb and sorted(da) == sorted(db) and sorted(ma) == sorted(mb)
        for k in da:
            same(da[k], db[k], f'prefetch vs inline data[{k}]')
        for k in ma:
            same(ma[k], mb[k], f'prefetch vs inline meta[{k}]')
        w = dataset.whole_frame(i, BG)
        assert ma['width'] == 48 and ma['height'] == 40 and ma['truth_u8'].shape == (40, 48, 3)
        same(ma['target_rgbs'], w['target_rgbs'], 'target_rgbs')
        same(ma['ray_alpha'], w['ray_alpha'], 'ray_alpha')
        same(ma['body'].astype(bool), w['ray_mask'].reshape(40, 48), 'body')
        same(ma['gt_alpha'], dataset.gt_alpha(i), 'gt_alpha')


def test_truth_panel_on_the_device_equals_the_host(dataset):
    got = dataset.truth_u8_device(1)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (40, 48, 3)
    same(got.cpu().numpy(), dataset.truth_u8(1), 'truth_u8')


# ---------------------------------------------------------------- 4. the entry points
def _run(tmp_path, script, *opts):
    cmd = [sys.executable, os.path.join(ROOT, script), '--cfg', CFG] + list(opts)
    out = subprocess.run(cmd, cwd=str(tmp_path), env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True,
                         timeout=170)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    return out.stdout


def test_train_py_on_a_dataset_resized_to_one_half(tmp_path, data_path):
    out = _run(tmp_path, 'train.py', 'train.dataset_path', data_path, *RESIZE_OPTS, 'N_samples', '32', 'train.maxiter', '6',
               'train.log_interval', '1', 'patch.size', '16', 'patch.N_patches', '4', 'progress.dump_interval', '3')
    assert '3 frames of 48 x 40' in out
    lines = [line for line in out.splitlines() if line.startswith('iter')]
    losses = [float(line.split('loss')[1].split()[0]) for line in lines]
    assert len(losses) == 6 and all(np.isfinite(losses))
    assert all(int(line.split('rays')[1].split()[0]) > 0 for line in lines)
    logdir = tmp_path / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf'
    assert os.path.exists(logdir / 'latest.tar') and os.path.exists(logdir / 'prog_000003.jpg')      # a progress mosaic too


@pytest.mark.parametrize('device_frames', ['True', 'False'], ids=['device-frames', 'host-frames'])
def test_eval_py_on_a_dataset_resized_to_one_half(device_frames, tmp_path, data_path):
    """device_frames False: the frames come from the numpy route (PreparedDataset.whole_frame, gt_alpha)."""
    import json
    from PIL import Image
    out = _run(tmp_path, 'eval.py', 'train.dataset_path', data_path, *RESIZE_OPTS, 'N_samples', '32', 'load_net', 'seeded',
               'device_frames', device_frames)
    assert 'targets are the dataset images (no teacher network): 3 frames' in out
    folder = tmp_path / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'seeded' / 'eval'
    rec = json.load(open(folder / 'metrics.json'))
    assert rec['n_frames'] == 3 and all(np.isfinite(f['psnr_full']) for f in rec['frames'])
    assert np.asarray(Image.open(folder / 'frame_000001.png')).shape == (40, 144, 3)


def test_run_py_freeview_with_the_truth_panel_on_a_dataset_resized_to_one_half(tmp_path, data_path):
    from PIL import Image
    from occnerf_amd.dataset import PreparedDataset
    _run(tmp_path, 'run.py', '--type', 'freeview', 'train.dataset_path', data_path, *RESIZE_OPTS, 'N_samples', '32',
         'load_net', 'seeded', 'render_frames', '2', 'freeview.frame_idx', '1', 'show_truth', 'True')
    folder = tmp_path / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'seeded' / 'freeview_1'
    assert sorted(os.listdir(folder)) == ['000000.png', '000001.png']
    ds = PreparedDataset(data_path, device=None, volume_size=4, resize_img_scale=0.5, resize_frames=True)
    panel = np.asarray(Image.open(folder / '000000.png'))
    assert panel.shape == (40, 96, 3)
    same(panel[:, 48:], ds.truth_u8(1), 'the truth half is the resized photograph')
