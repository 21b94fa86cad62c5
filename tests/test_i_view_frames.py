"""GPU: the rays-only row gather (occnerf_amd/csrc/view.hip, ops.view_frame), the loader around it
(ViewFrames.device_frames) and run.py --type freeview / backview on a prepared dataset.

The gather copies: everything it writes must be EQUAL to rays8[box] and np.nonzero(box) of what ops.gen_rays returned; how
close gen_rays is to numpy is tests/test_f_image_rays.py's business.  Where the device loader is compared with the host
loader every key must be equal for freeview / backview / allview, the rays included: their cameras are float64 and
gen_rays then performs numpy's operations in numpy's order (tests/test_h_whole_frame.py).  The tpose camera is float32:
rays <= 1e-6, near / far <= 2e-5 and the mask equal, tests/test_f_image_rays.py's rule.  The host frames themselves are
held to the reference in tests/test_view_frames_restatement.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import whole_frame_cases as cases
from tests.gpu_util import DEV, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml')


@pytest.fixture(scope='module')
def long_frame(tmp_path_factory):
    """gen_rays of the 300 x 37 dataset frame: two 256-pixel chunks per row, a width that is no multiple of 64."""
    from occnerf_amd import ops
    paths = cases.make_datasets(tmp_path_factory.mktemp('view_frame'), only=('long',))
    ds, frame = cases.open_case('two_chunks', paths, device=None)
    f, H, W = ds.frames[frame], ds.height, ds.width
    assert (H, W) == (37, 300)
    rays8, box = ops.gen_rays(f['K'], f['E'], H, W, f['dst_bbox_min'], f['dst_bbox_max'], DEV)
    torch.cuda.synchronize()
    per_row = box.cpu().numpy().reshape(H, W).sum(1)
    assert per_row.max() > 256 and 0 < per_row.sum() < H * W
    return rays8, box, rays8.cpu().numpy(), H, W


def to_numpy(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def compare_rows(got, rays8, box):
    compact = rays8[box]
    same(got['ray_index'], np.nonzero(box)[0].astype(np.int64), 'ray_index')
    same(got['rays'][0], compact[:, 0:3], 'rays_o')
    same(got['rays'][1], compact[:, 3:6], 'rays_d')
    same(got['near'], compact[:, 6:7], 'near')
    same(got['far'], compact[:, 7:8], 'far')


@pytest.mark.parametrize('kind', ['box', 'zeros', 'ones', 'bernoulli'])
def test_gather_equals_the_compaction_of_rays8(kind, long_frame):
    from occnerf_amd import ops
    rays8, box, rays8_np, H, W = long_frame
    box_np = {'box': box.cpu().numpy().astype(bool), 'zeros': np.zeros(H * W, bool), 'ones': np.ones(H * W, bool),
              'bernoulli': np.random.RandomState(7).rand(H * W) < 0.5}[kind]
    mask = torch.from_numpy(box_np.astype(np.uint8)).to(DEV)
    out = ops.view_frame(rays8, mask, H, W)
    assert sorted(out) == ['far', 'near', 'ray_index', 'rays']
    got = to_numpy(out)
    R = int(box_np.sum())
    assert (kind == 'zeros') == (R == 0) and (kind == 'ones') == (R == H * W)
    assert got['ray_index'].shape == (R,) and got['ray_index'].dtype == np.int64 and got['rays'].shape == (2, R, 3)
    assert got['near'].shape == got['far'].shape == (R, 1) and got['rays'].dtype == np.float32
    compare_rows(got, rays8_np, box_np)
    # the loader's form of the call: row_start and R from whole_frame_count
    row_start = ops.whole_frame_count(mask, H, W)
    assert int(row_start[H].item()) == R
    again = to_numpy(ops.view_frame(rays8, mask, H, W, row_start=row_start, R=R))
    for k in got:
        same(again[k], got[k], f'row_start given: {k}')


def test_a_callers_R_below_the_scan_total_writes_nothing_past_row_R(long_frame):
    from occnerf_amd import _lib, ops
    rays8, box, rays8_np, H, W = long_frame
    box_np = box.cpu().numpy().astype(bool)
    row_start = ops.whole_frame_count(box, H, W)
    total = int(row_start[H].item())
    starts = row_start.cpu().numpy()
    last = int(np.nonzero(np.diff(starts) > 1)[0][-1])          # the last row with more than one hit
    R = int(starts[last]) + 1                                  # ends inside that row
    assert 0 < R < total and R not in starts.tolist()
    idx = torch.full((total,), -7, device=DEV, dtype=torch.int64)
    rays = torch.full((2 * total * 3,), -7.0, device=DEV)
    near, far = torch.full((total,), -7.0, device=DEV), torch.full((total,), -7.0, device=DEV)
    with torch.cuda.device(DEV):
        rc = _lib.lib().occnerf_view_frame_gather(rays8.data_ptr(), box.data_ptr(), H, W, row_start.data_ptr(), R,
                                                  idx.data_ptr(), rays.data_ptr(), near.data_ptr(), far.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, 'view_frame_gather')
    torch.cuda.synchronize()
    compact = rays8_np[box_np][:R]
    same(idx.cpu().numpy()[:R], np.nonzero(box_np)[0][:R].astype(np.int64), 'ray_index below R')
    same(rays.cpu().numpy()[:6 * R].reshape(2, R, 3), np.stack([compact[:, 0:3], compact[:, 3:6]]), 'rays[2,R,3] below R')
    same(near.cpu().numpy()[:R], compact[:, 6], 'near below R')
    same(far.cpu().numpy()[:R], compact[:, 7], 'far below R')
    assert (idx[R:] == -7).all() and (rays[6 * R:] == -7).all() and (near[R:] == -7).all() and (far[R:] == -7).all()


def test_view_frame_refuses_bad_arguments(long_frame):
    from occnerf_amd import _lib, ops
    rays8, box, _, H, W = long_frame
    lib = _lib.lib()
    row_start = ops.whole_frame_count(box, H, W)
    R = int(row_start[H].item())
    out = ops.view_frame(rays8, box, H, W, row_start=row_start, R=R)
    p = [rays8.data_ptr(), box.data_ptr(), H, W, row_start.data_ptr(), R, out['ray_index'].data_ptr(),
         out['rays'].data_ptr(), out['near'].data_ptr(), out['far'].data_ptr(), None]

    def refused(changes, word):
        args = list(p)
        for i, v in changes.items():
            args[i] = v
        assert lib.occnerf_view_frame_gather(*args) != 0, changes
        msg = lib.occnerf_last_error().decode()
        assert 'view_frame_gather' in msg and word in msg, (changes, msg)

    for i in (0, 1, 4):
        refused({i: None}, 'null argument')
    for i in (6, 7, 8, 9):
        refused({i: None}, 'null ray output')
    refused({2: 0}, 'bad image size')
    refused({3: -1}, 'bad image size')
    refused({2: 1 << 14, 3: 1 << 14}, 'bad image size')         # H * W = 2^28
    refused({5: -1}, 'outside')
    refused({5: H * W + 1}, 'outside')
    assert lib.occnerf_view_frame_gather(*[v if i < 5 else (0 if i == 5 else None) for i, v in enumerate(p)]) == 0   # R = 0
    # the wrapper's own checks
    with pytest.raises(RuntimeError, match='rays8 must be a CUDA'):
        ops.view_frame(rays8.cpu(), box, H, W)
    with pytest.raises(RuntimeError, match='box_mask must be torch.uint8'):
        ops.view_frame(rays8, box.bool(), H, W)
    with pytest.raises(RuntimeError, match='rays8 must be a contiguous'):
        ops.view_frame(torch.empty(8, H * W, device=DEV).t(), box, H, W)
    with pytest.raises(RuntimeError, match='are not those of a'):
        ops.view_frame(rays8, box, H, W + 1)
    with pytest.raises(RuntimeError, match=r'must be in \[1, 2\^28\)'):
        ops.view_frame(rays8, box, 1 << 14, 1 << 14)
    with pytest.raises(RuntimeError, match='come together'):
        ops.view_frame(rays8, box, H, W, R=R)
    with pytest.raises(RuntimeError, match='outside'):
        ops.view_frame(rays8, box, H, W, row_start=row_start, R=H * W + 1)
    with pytest.raises(RuntimeError, match='row_start must be int32'):
        ops.view_frame(rays8, box, H, W, row_start=row_start[:-1].contiguous(), R=R)
    torch.cuda.synchronize()


@pytest.fixture(scope='module')
def rig_dataset(tmp_path_factory):
    from occnerf_amd.dataset import PreparedDataset
    path = str(tmp_path_factory.mktemp('views') / 'rig')
    cases.load_tool().make_dataset(path, frames=4, width=48, height=40, seed=3, focal=900.0, all_cameras=23)
    return PreparedDataset(path, device=None, volume_size=4)


def _frames(loader, prefetch):
    out = []
    for data, key, meta in loader.device_frames(DEV, prefetch=prefetch, data_type=loader.kind):
        torch.cuda.synchronize()
        out.append(({k: v.cpu().numpy().copy() for k, v in data.items()}, key,
                    {k: (v.cpu().numpy().copy() if torch.is_tensor(v) else v) for k, v in meta.items()}))
    return out


def _host_frames(loader, monkeypatch):
    """The host loader through frames_to_device (`device_frames False`), tensors on the GPU."""
    from occnerf_amd import config, sequence
    cfg = config.default_cfg()
    cfg.device_frames = False
    monkeypatch.setattr(sequence, 'get_cfg', lambda: cfg)
    host = list(sequence.frames_to_device(loader, loader.kind, DEV))
    torch.cuda.synchronize()
    return host


@pytest.mark.parametrize('kind', ['freeview', 'backview', 'allview'])
def test_device_frames_prefetch_equals_inline_equals_the_host_loader(kind, rig_dataset, monkeypatch):
    from occnerf_amd.views import ViewFrames
    loader = ViewFrames(rig_dataset, kind, bgcolor=[30., 200., 90.], render_frames=6, frame_idx=1)
    n = {'freeview': 6, 'backview': 4, 'allview': 23}[kind]
    a, b = _frames(loader, True), _frames(loader, False)
    assert len(loader) == len(a) == len(b) == n
    for (da, ka, ma), (db, kb, mb) in zip(a, b):
        assert ka is None and kb is None and sorted(da) == sorted(db) and sorted(ma) == sorted(mb)
        assert sorted(ma) == ['frame_name', 'height', 'idx', 'ray_index', 'truth_u8', 'width']
        for k in da:
            same(da[k], db[k], f'prefetch vs inline data[{k}]')
        for k in ma:
            same(ma[k], mb[k], f'prefetch vs inline meta[{k}]')
    host = _host_frames(loader, monkeypatch)
    assert len(host) == n
    counts = []
    for i, ((dh, kh, mh), (da, ka, ma)) in enumerate(zip(host, a)):
        assert kh is None and sorted(dh) == sorted(da) and sorted(mh) == sorted(ma), (sorted(dh), sorted(da), sorted(mh))
        for k in dh:
            h = dh[k].cpu().numpy()
            assert h.dtype == da[k].dtype, k
            same(da[k], h, f'frame {i}: device vs host data[{k}]')
        for k in mh:
            same(ma[k], mh[k].cpu().numpy() if torch.is_tensor(mh[k]) else mh[k], f'frame {i}: device vs host meta[{k}]')
        src = loader.view(i)['src']
        same(ma['truth_u8'], rig_dataset.images[src], 'truth_u8 is the photograph')
        assert ma['frame_name'] == rig_dataset.framelist[src] and (ma['width'], ma['height'], ma['idx']) == (48, 40, i)
        counts.append(int(ma['ray_index'].size))
    assert min(counts) > 0 and len(set(counts)) > 1            # the cameras differ


def test_device_frames_of_tpose_at_32(rig_dataset, monkeypatch):
    from occnerf_amd.views import CanonicalSubject, ViewFrames
    loader = ViewFrames(CanonicalSubject(rig_dataset.dataset_path, volume_size=4), 'tpose', render_size=32)
    a, b = _frames(loader, True), _frames(loader, False)
    assert len(a) == len(b) == 1
    (da, ka, ma), (db, kb, mb) = a[0], b[0]
    assert ka is None and sorted(ma) == ['frame_name', 'height', 'idx', 'ray_index', 'width']        # no photograph
    for k in da:
        same(da[k], db[k], f'prefetch vs inline data[{k}]')
    same(ma['ray_index'], mb['ray_index'], 'prefetch vs inline ray_index')
    (dh, kh, mh), = _host_frames(loader, monkeypatch)
    assert sorted(dh) == sorted(da)
    same(ma['ray_index'], mh['ray_index'].cpu().numpy(), 'ray_index (the mask)')
    assert 0 < ma['ray_index'].size < 32 * 32
    for k, tol in (('rays', 1e-6), ('near', 2e-5), ('far', 2e-5)):
        err = float(np.abs(da[k] - dh[k].cpu().numpy()).max())
        print(f'   tpose 32 x 32 {k}: max |device - host| = {err:.3e}')
        assert da[k].shape == tuple(dh[k].shape) and err <= tol, (k, err)
    for k in dh:
        if k not in ('rays', 'near', 'far'):
            same(da[k], dh[k].cpu().numpy(), f'device vs host data[{k}]')


def test_device_frames_names_the_frame_whose_box_misses_the_image(rig_dataset):
    import copy
    from occnerf_amd.views import ViewFrames
    ds = copy.copy(rig_dataset)
    ds.frames = [dict(f) for f in rig_dataset.frames]
    ds.frames[2]['dst_bbox_min'] = ds.frames[2]['dst_bbox_min'] + 100.0
    ds.frames[2]['dst_bbox_max'] = ds.frames[2]['dst_bbox_max'] + 100.0
    ds._dev = None
    for prefetch in (True, False):
        it = ViewFrames(ds, 'backview', render_frames=6).device_frames(DEV, prefetch=prefetch)
        assert [next(it)[2]['frame_name'] for _ in range(2)] == ['frame_000000', 'frame_000001']
        with pytest.raises(ValueError, match='frame_000002'):
            next(it)
    torch.cuda.synchronize()


@pytest.mark.parametrize('kind', ['freeview', 'backview'])
def test_run_py_on_a_prepared_dataset(kind, tmp_path):
    """python run.py --type freeview / backview on a tool-made dataset: the reference's folder and file names, and with
    show_truth and show_alpha the panels [rgb, truth, alpha], the middle one the photograph byte for byte."""
    from PIL import Image
    path = str(tmp_path / 'data')
    cases.load_tool().make_dataset(path, frames=2, width=48, height=40, seed=31, focal=900.0)
    cmd = [sys.executable, os.path.join(ROOT, 'run.py'), '--cfg', CFG, '--type', kind, 'train.dataset_path', path,
           'resize_img_scale', '1.0', 'N_samples', '32', 'load_net', 'seeded', 'render_frames', '3', 'freeview.frame_idx', '1',
           'show_truth', 'True', 'show_alpha', 'True']
    out = subprocess.run(cmd, cwd=str(tmp_path), env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True,
                         timeout=170)
    assert out.returncode == 0, out.stderr[-3000:]
    folder = tmp_path / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'seeded' / \
        {'freeview': 'freeview_1', 'backview': 'backview'}[kind]
    names = {'freeview': ['000000.png', '000001.png', '000002.png'], 'backview': ['000000.png', '000001.png']}[kind]
    assert sorted(os.listdir(folder)) == names
    for i, name in enumerate(names):
        photo = np.asarray(Image.open(os.path.join(path, 'images', 'frame_%06d.png' % (1 if kind == 'freeview' else i))))
        panel = np.asarray(Image.open(folder / name))
        assert panel.shape == (40, 144, 3)
        same(panel[:, 48:96], photo, f'{name}: the truth third is the photograph')
        alpha = panel[:, 96:]
        assert (alpha[..., 0] == alpha[..., 1]).all() and (alpha[..., 0] == alpha[..., 2]).all()      # the grey alpha panel
        assert not np.array_equal(panel[:, :48], photo)
