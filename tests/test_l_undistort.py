"""GPU: the undistortion kernel (occnerf_amd/csrc/undistort.hip, ops.undistort_u8), the dataset open around it
(PreparedDataset(prepare_frames=True) with a device), what reads the prepared frames downstream, the allview truth panel of
a distorted rig, and train.py / run.py on a distorted dataset.

The kernel performs occnerf_amd/undistort.py's IEEE operations in its order -- float64, one rounding per operator, then
integers -- so EVERY comparison in this file is equality.  Each kernel case also prints how close 32 u and 32 v come to a
rounding tie, so that a mismatch could be told apart from a tie."""
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from occnerf_amd.undistort import source_coordinates, undistort_u8
from tests import train_batch_restatement as tbr
from tests import undistort_cases as uc
from tests import whole_frame_restatement as wfr
from tests.gpu_util import DEV, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml')
CROP = [31, 26]

# name -> (H, W, K, D, windows): the two cameras of the CPU file; a row longer than one 256-thread chunk whose width is no
# multiple of 64 or 4; one pixel
KERNEL_CASES = {
    'A': uc.case('A') + ([None, (7, 13, 33, 51), (95, 127, 1, 1)],),
    'B': uc.case('B') + ([None, (1, 3, 37, 65), (0, 0, 1, 72)],),
    'B4': uc.case('B')[:3] + (np.array(uc.CAMERAS['B'][2][:4]), [None, (3, 5, 9, 11)]),
    'row': (9, 300, uc.matrix(260., 255., 151.7, 4.3), np.array([-0.31, 0.12, 0.002, -0.001, -0.04]), [None, (1, 1, 7, 297)]),
    'pixel': (1, 1, uc.matrix(2., 2., 0.2, 0.1), np.array([0.3, 0.1, 0.01, 0.02]), [None]),
}


def tie_distance(H, W, K, D):
    u, v = source_coordinates(H, W, K, D)
    t = np.concatenate([(u * 32).ravel(), (v * 32).ravel()])
    t = t[np.isfinite(t) & (np.abs(t) < 2.0 ** 31)]
    return float(np.abs(np.abs(t - np.floor(t)) - 0.5).min())


@pytest.mark.parametrize('name', list(KERNEL_CASES))
def test_kernel_equals_the_numpy_definition(name):
    from occnerf_amd import ops
    H, W, K, D, windows = KERNEL_CASES[name]
    rng = np.random.RandomState(len(name) + H)
    img = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)                # not smooth: every weight pair occurs
    mask = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    print(f'\n   {name}: {W} x {H}, {len(D)} coefficients; smallest distance of 32u / 32v from a tie {tie_distance(H, W, K, D):.3e}')
    d_img, d_mask = torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV)
    for window in windows:
        want_img, want_mask = undistort_u8(img, K, D, window), undistort_u8(mask, K, D, window)
        got_img, got_mask = ops.undistort_u8(d_img, d_mask, K, D, window)
        only_img, none = ops.undistort_u8(d_img, None, K, D, window)          # a null mask
        torch.cuda.synchronize()
        assert none is None and got_img.dtype == torch.uint8 and tuple(got_img.shape) == want_img.shape
        same(got_img.cpu().numpy(), want_img, f'{name} {window}: image')
        same(got_mask.cpu().numpy(), want_mask, f'{name} {window}: mask')
        same(only_img.cpu().numpy(), want_img, f'{name} {window}: image without a mask')
    if name in ('A', 'B'):                                  # the smooth image of the CPU file and the coefficient shapes
        smooth = uc.smooth_image(H, W)
        got = ops.undistort_u8(torch.from_numpy(smooth).to(DEV), None, K, D.reshape(-1, 1))[0]
        same(got.cpu().numpy(), undistort_u8(smooth, K, D), f'{name}: the smooth image')


def test_kernel_writes_only_the_window_and_refuses_bad_arguments():
    from occnerf_amd import ops
    H, W, K, D = uc.case('B')
    img = torch.from_numpy(np.random.RandomState(3).randint(0, 256, size=(H, W, 3)).astype(np.uint8)).to(DEV)
    # the outputs are slices of one guarded buffer each: nothing but the window's bytes changes
    h, w = 9, 11
    bufs = [torch.full((h * w * 3 + 128,), 0xA5, dtype=torch.uint8, device=DEV) for _ in range(2)]
    out = tuple(b[64:64 + h * w * 3].view(h, w, 3) for b in bufs)
    ops.undistort_u8(img, img, K, D, window=(3, 5, h, w), out=out)
    torch.cuda.synchronize()
    for b in bufs:
        same(b[64:-64].view(h, w, 3).cpu().numpy(), undistort_u8(img.cpu().numpy(), K, D, (3, 5, h, w)), 'window')
        assert (b[:64] == 0xA5).all() and (b[-64:] == 0xA5).all()
    with pytest.raises(RuntimeError, match='image must be a CUDA'):
        ops.undistort_u8(img.cpu(), None, K, D)
    with pytest.raises(RuntimeError, match='mask must be torch.uint8'):
        ops.undistort_u8(img, img.float(), K, D)
    with pytest.raises(ValueError, match='window'):
        ops.undistort_u8(img, None, K, D, window=(0, 0, H, W + 1))
    with pytest.raises(NotImplementedError, match='tilt'):
        ops.undistort_u8(img, None, K, np.zeros(14))
    skewed = K.copy()
    skewed[0, 1] = 1e-3
    with pytest.raises(NotImplementedError, match='skew'):
        ops.undistort_u8(img, None, skewed, D)
    with pytest.raises(RuntimeError, match='out must be'):
        ops.undistort_u8(img, None, K, D, out=(torch.empty(H, W + 1, 3, dtype=torch.uint8, device=DEV), None))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the dataset
@pytest.fixture(scope='module')
def tool_path(tmp_path_factory):
    """48 x 40, 5 frames with 'distortions'; frame 3's camera has lost the key."""
    path = uc.make_tool_dataset(tmp_path_factory.mktemp('undistort_gpu') / 'data')
    uc.edit_pickle(path, 'cameras.pkl', lambda cams: cams['frame_000003'].pop('distortions'))
    return path


def open_dataset(path, device, crop=CROP):
    from occnerf_amd.dataset import PreparedDataset
    return PreparedDataset(path, device=device, volume_size=4, occlude=True, occlusion=uc.BAND, prepare_frames=True,
                           crop_image_scale=crop)


@pytest.fixture(scope='module')
def opened(tool_path):
    return open_dataset(tool_path, None), open_dataset(tool_path, DEV)


@pytest.mark.parametrize('crop', [CROP, [-1, -1]], ids=['cropped', 'whole'])
def test_open_with_a_device_equals_the_host_open(crop, tool_path, opened):
    host, dev = opened if crop == CROP else (open_dataset(tool_path, None, crop), open_dataset(tool_path, DEV, crop))
    assert (host.height, host.width) == (dev.height, dev.width) == ((31, 26) if crop == CROP else (40, 48))
    assert len(host) == len(dev) == 5 and host.epoch_frames == dev.epoch_frames
    for i in range(5):
        same(dev.images[i], host.images[i], f'frame {i}: image')
        same(dev.alphas[i], host.alphas[i], f'frame {i}: mask')
        same(dev.frames[i]['K'], host.frames[i]['K'], f'frame {i}: K')
        assert dev.frames[i]['empty'] == host.frames[i]['empty']
        same(dev._dev['image'][i].cpu().numpy(), host.images[i], f'frame {i}: the resident image')
        same(dev._dev['alpha'][i].cpu().numpy(), host.alphas[i], f'frame {i}: the resident mask')
    assert not np.array_equal(host.images[0], host.images[3])


def test_whole_frame_on_the_device_equals_the_host_frame(opened):
    """One device_frames whole frame of the distorted, cropped dataset against whole_frame(), as tests/test_h_whole_frame.py
    compares them."""
    from occnerf_amd.dataset import WholeFrames
    host, dev = opened
    bgcolor = [30., 200., 90.]
    data, key, meta = next(iter(WholeFrames(dev, bgcolor).device_frames(DEV, prefetch=False)))
    torch.cuda.synchronize()
    w = host.whole_frame(0, bgcolor)
    assert (meta['height'], meta['width']) == (31, 26) == (w['img_height'], w['img_width'])
    assert 0 < int(w['ray_mask'].sum())
    same(meta['ray_index'].cpu().numpy(), np.nonzero(w['ray_mask'])[0].astype(np.int64), 'ray_index')
    for k in ('rays', 'near', 'far', 'target_rgbs', 'ray_alpha'):
        same(data[k].cpu().numpy(), w[k], k)
    truth, gt_vis, gt_alpha = wfr.maps(w, host.alphas[0], bgcolor)
    same(meta['truth_u8'].cpu().numpy(), truth, 'truth_u8')
    same(meta['gt_vis'].cpu().numpy(), gt_vis, 'gt_vis')
    same(meta['gt_alpha'].cpu().numpy(), gt_alpha, 'gt_alpha')
    same(meta['body'].cpu().numpy().astype(bool), w['ray_mask'].reshape(31, 26), 'body')


def test_patch_batch_equals_the_host_batch_for_the_same_draws(opened, tmp_path):
    """One batch of PatchBatchLoader on the distorted, cropped dataset against the restatement of the reference's loader
    (tests/train_batch_restatement.py), which neither undistorts nor crops: it is given the PREPARED frames as a dataset of
    their own -- the prepared PNGs and the prepared K, no 'distortions' -- and the draws the loader made."""
    from PIL import Image
    from occnerf_amd.dataset import PatchBatchLoader
    from tests.test_g_train_batch import compare
    host, dev = opened
    path = str(tmp_path / 'prepared')
    os.makedirs(os.path.join(path, 'images'))
    os.makedirs(os.path.join(path, 'masks'))
    for name in ('mesh_infos.pkl', 'canonical_joints.pkl'):
        with open(os.path.join(host.dataset_path, name), 'rb') as f, open(os.path.join(path, name), 'wb') as g:
            g.write(f.read())
    cams = {}
    for i, name in enumerate(host.framelist):
        Image.fromarray(host.images[i], 'RGB').save(os.path.join(path, 'images', name + '.png'))
        Image.fromarray(host.alphas[i], 'RGB').save(os.path.join(path, 'masks', name + '.png'))
        cams[name] = {'intrinsics': host.frames[i]['K'], 'extrinsics': host.frames[i]['extrinsics']}
    with open(os.path.join(path, 'cameras.pkl'), 'wb') as f:
        pickle.dump(cams, f, protocol=4)
    loader = PatchBatchLoader(dev, n_patches=4, size=16, bgcolor=None, seed=5, prefetch=False)
    b = next(loader)
    torch.cuda.synchronize()
    got = {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in b.items()}
    got['n_rows'] = np.array([b['n_rows']])
    rs = tbr.Restatement(path, N_patches=4, size=16, volume_size=4)           # the band is already in the prepared masks
    _, _, subject, off = rs.frame_masks(b['frame'])
    r = rs.getitem(b['frame'], b['bgcolor'], tbr.draws_from_uniforms(b['u'], subject, off, 0.8))
    from occnerf_amd import ops
    f = dev.frames[b['frame']]
    rays8, box = ops.gen_rays(f['K'], f['E'], dev.height, dev.width, f['dst_bbox_min'], f['dst_bbox_max'], DEV)
    torch.cuda.synchronize()
    R = b['n_rows']
    full = dict(got)                                        # compare() reads whole buffers and slices them by the row count
    compare(full, rays8.cpu().numpy(), box.cpu().numpy().astype(bool), r, 4, 16)
    assert R > 0 and (dev.height, dev.width) == (31, 26)


# ---------------------------------------------------------------- allview
@pytest.fixture(scope='module')
def rig_path(tmp_path_factory):
    """A 6-camera rig ('wild' in the path) whose cameras each have a lens and a principal point of their own."""
    path = uc.make_tool_dataset(tmp_path_factory.mktemp('undistort_wild') / 'rig', frames=2, all_cameras=6)

    def vary(rigs):
        for rig in rigs.values():
            rig['distortions'] = rig['distortions'] * (1.0 + 0.1 * np.arange(6))[:, None]
            rig['intrinsics'] = rig['intrinsics'].copy()
            rig['intrinsics'][:, 0, 2] += 0.25 * np.arange(6)
    uc.edit_pickle(path, 'all_cameras.pkl', vary)
    return path


def photograph(path, name):
    from PIL import Image
    return np.array(Image.open(os.path.join(path, 'images', name + '.png')).convert('RGB'))


@pytest.mark.parametrize('prefetch', [True, False], ids=['prefetch', 'inline'])
def test_allview_truth_is_the_raw_photograph_through_each_rig_camera(prefetch, rig_path, tmp_path):
    from occnerf_amd.dataset import PreparedDataset
    from occnerf_amd.views import ViewFrames
    ds = PreparedDataset(rig_path, device=None, volume_size=4, prepare_frames=True)
    with open(os.path.join(rig_path, 'all_cameras.pkl'), 'rb') as f:
        rig = pickle.load(f)['frame_000001']
    photo = photograph(rig_path, 'frame_000001')
    views = ViewFrames(ds, 'allview', src_type='wild', frame_idx=1)
    panels = []
    for i, (data, key, meta) in enumerate(views.device_frames(DEV, prefetch=prefetch)):
        torch.cuda.synchronize()
        panels.append(meta['truth_u8'].cpu().numpy())
        same(panels[i], undistort_u8(photo, rig['intrinsics'][i], rig['distortions'][i]), f'camera {i}: truth_u8')
        same(panels[i], views.frame(i)['truth_u8'], f'camera {i}: the host dict')
    assert len(panels) == 6 and not np.array_equal(panels[0], panels[5])
    assert all('truth_u8' not in meta for _, _, meta in
               ViewFrames(ds, 'allview', src_type='wild', frame_idx=1, truth=False).device_frames(DEV, prefetch=prefetch))
    # a rig without the key: the resident photograph, as before
    plain_path = str(tmp_path / 'plain_wild')
    shutil.copytree(rig_path, plain_path)
    uc.edit_pickle(plain_path, 'all_cameras.pkl', lambda rigs: [r.pop('distortions') for r in rigs.values()])
    ds = PreparedDataset(plain_path, device=None, volume_size=4, prepare_frames=True)
    n = 0
    for data, key, meta in ViewFrames(ds, 'allview', src_type='wild', frame_idx=1).device_frames(DEV, prefetch=prefetch):
        torch.cuda.synchronize()
        same(meta['truth_u8'].cpu().numpy(), ds.images[1], 'a rig without distortions shows the resident photograph')
        n += 1
    assert n == 6
    torch.cuda.synchronize()


# ---------------------------------------------------------------- entry points
def test_train_py_on_a_distorted_dataset(tmp_path):
    path = uc.make_tool_dataset(tmp_path / 'data', frames=3, width=64, height=64)
    cmd = [sys.executable, os.path.join(ROOT, 'train.py'), '--cfg', CFG, 'train.dataset_path', path, 'resize_img_scale', '1.0',
           'N_samples', '32', 'train.maxiter', '2', 'train.log_interval', '1', 'patch.size', '16', 'patch.N_patches', '4',
           'crop_image_scale', '[49, 40]', 'train.lossweights', "{'mse': 0.2, 'comp': 1.0}", 'progress.dump_interval', '0']
    out = subprocess.run(cmd, cwd=str(tmp_path), env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True,
                         timeout=170)
    print(out.stdout)
    assert out.returncode == 0, out.stderr[-3000:]
    assert '3 frames of 40 x 49' in out.stdout, out.stdout[-2000:]
    lines = [line for line in out.stdout.splitlines() if line.startswith('iter')]
    losses = [float(line.split('loss')[1].split()[0]) for line in lines]
    assert len(losses) == 2 and all(np.isfinite(losses))


def test_run_py_allview_on_a_distorted_dataset(tmp_path):
    """The truth third of two of the rig's panels is the raw photograph undistorted for that camera, byte for byte."""
    from PIL import Image
    path = uc.make_tool_dataset(tmp_path / 'wild_data', frames=2, all_cameras=6)
    cmd = [sys.executable, os.path.join(ROOT, 'run.py'), '--cfg', CFG, '--type', 'allview', 'train.dataset_path', path,
           'resize_img_scale', '1.0', 'N_samples', '32', 'load_net', 'seeded', 'freeview.frame_idx', '1',
           'freeview.src_type', 'wild', 'show_truth', 'True']
    out = subprocess.run(cmd, cwd=str(tmp_path), env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True,
                         timeout=170)
    assert out.returncode == 0, out.stderr[-3000:]
    folder = tmp_path / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'seeded' / 'allview_1'
    assert sorted(os.listdir(folder)) == ['%06d.png' % i for i in range(6)]
    with open(os.path.join(path, 'all_cameras.pkl'), 'rb') as f:
        rig = pickle.load(f)['frame_000001']
    photo = photograph(path, 'frame_000001')
    for i in (0, 5):
        panel = np.asarray(Image.open(folder / ('%06d.png' % i)))
        assert panel.shape == (40, 96, 3)
        same(panel[:, 48:], undistort_u8(photo, rig['intrinsics'][i], rig['distortions'][i]), f'camera {i}: the truth half')
