"""CPU: the cameras derived from a prepared dataset (occnerf_amd/views.py: freeview, backview, allview, tpose) against the
recording of the UNMODIFIED reference datasets (tests/golden/view_frames_ref.npz, tools/record_view_frames_golden.py).

Both sides are numpy doing the same operations on float64 cameras, so ray_mask, near, far, the box constants, cnl_gtfms
and dst_posevec must be EQUAL (motion_weights_priors: see compare_priors), and rays equal to the recording's .astype('float32') (the reference hands float64 rays to a
DataLoader whose consumer casts them; tests/test_train_batch_restatement.py applies the same rule).  dst_Rs / dst_Ts are
held to 1e-6 absolute, the tolerance of tests/test_a_rows.py row a2.  The tpose camera is float32: rays <= 1e-6, near / far
<= 2e-5 and the mask equal, tests/test_f_image_rays.py's rule for float32 cameras.  The device side of the same frames is
tests/test_i_view_frames.py."""
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests.train_batch_cases import load_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'view_frames_ref.npz')
EXACT_KEYS = ('cnl_gtfms', 'cnl_bbox_min_xyz', 'cnl_bbox_max_xyz', 'cnl_bbox_scale_xyz', 'dst_posevec', 'bgcolor')


def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def golden_tool_args(g):
    frames, width, height, seed, focal, all_cameras = g['meta.tool_args']
    return {'frames': int(frames), 'width': int(width), 'height': int(height), 'seed': int(seed), 'focal': float(focal),
            'all_cameras': int(all_cameras)}


def golden_cfg(g):
    render_frames, frame_idx, bbox_offset, scale, volume_size = g['meta.config']
    return {'render_frames': int(render_frames), 'frame_idx': int(frame_idx), 'bbox_offset': float(bbox_offset),
            'resize_img_scale': float(scale), 'volume_size': int(volume_size)}


def golden_plan(g):
    out = []
    for line in g['meta.plan']:
        tag, kind, src_type, frames = str(line).split(':')
        out.append((tag, kind, src_type, [int(f) for f in frames.split(',')]))
    return out


@pytest.fixture(scope='module')
def golden_dataset(tmp_path_factory):
    from occnerf_amd.dataset import PreparedDataset
    g = golden()
    path = str(tmp_path_factory.mktemp('view_frames_dataset'))
    load_tool().make_dataset(path, **golden_tool_args(g))
    c = golden_cfg(g)
    ds = PreparedDataset(path, device=None, bbox_offset=c['bbox_offset'], volume_size=c['volume_size'],
                         resize_img_scale=c['resize_img_scale'])
    return g, path, ds


def open_views(ds, kind, src_type, c, **kw):
    from occnerf_amd.views import ViewFrames
    return ViewFrames(ds, kind, src_type=src_type, render_frames=c['render_frames'], frame_idx=c['frame_idx'],
                      bbox_offset=c['bbox_offset'], **kw)


def compare_priors(got, want, tag):
    """Same bbox_offset and volume size on both sides, yet not equal: synth.approx_gaussian_bone_volumes restates
    body_util.py:274-350 with other float32 intermediates (measured: 950 of 12 800 entries differ, the largest by 1.64e-7),
    so the volume is held to 1e-5, what tests/test_a_rows.py and tests/test_train_batch_restatement.py hold it to."""
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    assert float(np.abs(got - want).max()) <= 1e-5, (tag, float(np.abs(got - want).max()))


def compare_frame(got, g, prefix, tag):
    """A host frame of ViewFrames against the recorded reference frame: everything but dst_Rs / dst_Ts equal."""
    assert got['ray_mask'].dtype == np.bool_ and np.array_equal(got['ray_mask'], g[prefix + 'ray_mask']), prefix
    for k in ('near', 'far'):
        assert got[k].dtype == g[prefix + k].dtype == np.float32 and np.array_equal(got[k], g[prefix + k]), (prefix, k)
    assert g[prefix + 'rays'].dtype == np.float64 and got['rays'].dtype == np.float32
    assert np.array_equal(got['rays'], g[prefix + 'rays'].astype('float32')), prefix
    for k in EXACT_KEYS:
        assert got[k].dtype == g[prefix + k].dtype and np.array_equal(got[k], g[prefix + k]), (prefix, k)
    for k in ('dst_Rs', 'dst_Ts'):
        err = float(np.abs(got[k] - g[prefix + k]).max())
        assert got[k].shape == g[prefix + k].shape and got[k].dtype == g[prefix + k].dtype and err <= 1e-6, (prefix, k, err)
    compare_priors(got['motion_weights_priors'], g[f'{tag}.motion_weights_priors'], tag)
    assert [got['img_width'], got['img_height']] == g[prefix + 'size'].tolist()


def test_freeview_backview_allview_equal_the_recorded_reference(golden_dataset):
    g, path, ds = golden_dataset
    c = golden_cfg(g)
    seen = 0
    for tag, kind, src_type, frames in golden_plan(g):
        if kind == 'tpose':
            continue
        vf = open_views(ds, kind, src_type, c)
        assert len(vf) == int(g[f'{tag}.len']), tag
        assert vf.dataset.avg_betas.shape == (10,)
        for i in frames:
            got = vf.frame(i)
            compare_frame(got, g, f'{tag}.f{i}.', tag)
            assert got['frame_name'] == str(g[f'{tag}.f{i}.frame_name'])
            # the truth panel: the reference's to_8b_image(img / 255.) is the photograph itself
            assert got['truth_u8'].dtype == np.uint8 and np.array_equal(got['truth_u8'], g[f'{tag}.f{i}.truth_u8'])
            assert 0 < got['ray_mask'].sum() < got['ray_mask'].size
            seen += 1
    assert seen == 11
    # the orbit is not a no-op, and the two source types turn about different axes
    a, b = open_views(ds, 'freeview', 'zju_mocap', c), open_views(ds, 'freeview', 'wild', c)
    assert not np.array_equal(a.frame(0)['ray_mask'], a.frame(1)['ray_mask'])
    assert np.array_equal(a.frame(0)['ray_mask'], b.frame(0)['ray_mask'])
    assert not np.array_equal(a.frame(1)['ray_mask'], b.frame(1)['ray_mask'])


def test_tpose_equals_the_recorded_reference_at_512(golden_dataset):
    from occnerf_amd.views import CanonicalSubject, ViewFrames
    g, path, _ = golden_dataset
    c = golden_cfg(g)
    stride = int(g['meta.tpose_row_stride'])
    vf = ViewFrames(CanonicalSubject(path, c['bbox_offset'], c['volume_size']), 'tpose', render_size=512)
    assert len(vf) == int(g['tpose.len']) == 1 and vf.dataset.avg_betas.shape == (10,)
    got = vf.frame(0)
    assert 'truth_u8' not in got                               # there is no photograph
    mask = np.unpackbits(g['tpose.f0.ray_mask'])[:512 * 512].astype(bool)
    assert np.array_equal(got['ray_mask'], mask) and int(got['ray_mask'].sum()) == int(g['tpose.f0.ray_count'])
    errs = {'rays': float(np.abs(got['rays'][:, ::stride] - g['tpose.f0.rays']).max()),
            'near': float(np.abs(got['near'][::stride] - g['tpose.f0.near']).max()),
            'far': float(np.abs(got['far'][::stride] - g['tpose.f0.far']).max())}
    print('\n   tpose 512 x 512, every %dth row of %d: max |diff| %s' % (stride, int(mask.sum()), errs))
    assert got['rays'][:, ::stride].shape == g['tpose.f0.rays'].shape and got['rays'].dtype == np.float32
    assert errs['rays'] <= 1e-6 and errs['near'] <= 2e-5 and errs['far'] <= 2e-5
    for k in EXACT_KEYS:
        assert got[k].dtype == g['tpose.f0.' + k].dtype and np.array_equal(got[k], g['tpose.f0.' + k]), k
    for k in ('dst_Rs', 'dst_Ts'):
        assert float(np.abs(got[k] - g['tpose.f0.' + k]).max()) <= 1e-6, k
    compare_priors(got['motion_weights_priors'], g['tpose.motion_weights_priors'], 'tpose')
    assert np.all(got['dst_posevec'] == np.float32(1e-2))


def test_the_truth_panel_maps_all_256_levels_to_themselves():
    """to_8b_image(img / 255.) -- freeview.py:187 then run.py's truth panel -- is the identity on uint8, so `truth_u8` may be
    the resident photograph."""
    from occnerf_amd.image import to_8b_image
    levels = np.arange(256, dtype=np.uint8)
    assert np.array_equal(to_8b_image(levels / 255.), levels)
    assert np.array_equal(to_8b_image((levels / 255.).reshape(16, 16, 1).repeat(3, 2)).reshape(256, 3)[:, 1], levels)


def test_backview_keeps_the_first_frames_reference_camera_under_skip(golden_dataset):
    from occnerf_amd.dataset import apply_global_tfm_to_camera
    from occnerf_amd.views import ROT_CAM_PARAMS, rotate_camera_by_frame_idx
    g, path, ds = golden_dataset
    c = golden_cfg(g)
    vf = open_views(ds, 'backview', 'zju_mocap', c, skip=3)
    assert len(vf) == 2 and [vf.view(i)['frame_name'] for i in range(2)] == ['frame_000000', 'frame_000003']
    # frame 3 seen from frame 0's reference camera: what the reference recorded walking all four frames
    compare_frame(vf.frame(1), g, 'backview.f3.', 'backview')
    # asked for in the other order the camera is still the first frame's
    other = open_views(ds, 'backview', 'zju_mocap', c, skip=3)
    assert np.array_equal(other.view(1)['E'], vf.view(1)['E']) and other.view(1)['K'] is ds.frames[0]['K']
    E_ref = rotate_camera_by_frame_idx(ds.frames[0]['extrinsics'], c['render_frames'] // 2, trans=None,
                                       period=c['render_frames'], **ROT_CAM_PARAMS['zju_mocap'])
    assert np.array_equal(vf.view(1)['E'], apply_global_tfm_to_camera(E_ref, ds.frames[3]['Rh_vec'], ds.frames[3]['Th']))
    own = rotate_camera_by_frame_idx(ds.frames[3]['extrinsics'], c['render_frames'] // 2, trans=None,
                                     period=c['render_frames'], **ROT_CAM_PARAMS['zju_mocap'])
    assert not np.array_equal(E_ref, own)                      # frame 3's own camera would have given another view
    assert len(open_views(ds, 'backview', 'zju_mocap', c, skip=1, maxframes=3)) == 3


def _copy_dataset(src, dst, drop=()):
    shutil.copytree(src, dst, ignore=shutil.ignore_patterns(*drop) if drop else None)
    return dst


def test_allview_reads_the_rig_and_names_the_file_it_misses(golden_dataset, tmp_path):
    from occnerf_amd.dataset import PreparedDataset
    g, path, ds = golden_dataset
    c = golden_cfg(g)
    kw = dict(device=None, bbox_offset=c['bbox_offset'], volume_size=4)
    bare = _copy_dataset(path, str(tmp_path / 'bare'), drop=('all_cameras.pkl',))
    with pytest.raises(FileNotFoundError, match='all_cameras.pkl'):
        open_views(PreparedDataset(bare, **kw), 'allview', 'zju_mocap', c)
    few = str(tmp_path / 'few')
    args = dict(golden_tool_args(g), all_cameras=5)
    load_tool().make_dataset(few, **args)
    with pytest.raises(ValueError, match=r'all_cameras\.pkl.*5 cameras.*23'):
        open_views(PreparedDataset(few, **kw), 'allview', 'zju_mocap', c)
    # 'wild' in the dataset path: 6 cameras (allview.py:69), so the same 5 are still too few and 23 are plenty
    with pytest.raises(ValueError, match=r'all_cameras\.pkl.*5 cameras.*6'):
        open_views(PreparedDataset(_copy_dataset(few, str(tmp_path / 'wild_few')), **kw), 'allview', 'wild', c)
    wild = PreparedDataset(_copy_dataset(path, str(tmp_path / 'wild_rig')), **kw)
    assert len(open_views(wild, 'allview', 'wild', c)) == 6
    # all_mesh_infos.pkl (has_all_mesh): the body indexed per camera.  With every camera given the frame's own body the
    # frames are the ones without the file
    with open(os.path.join(path, 'mesh_infos.pkl'), 'rb') as f:
        info = pickle.load(f)
    rep = {n: {k: np.repeat(np.asarray(v)[None], 23, axis=0) for k, v in d.items()} for n, d in info.items()}
    rep['frame_000001']['Th'][7] += np.float32(0.05)           # ... except camera 7, whose body is moved
    mesh = _copy_dataset(path, str(tmp_path / 'mesh'))
    with open(os.path.join(mesh, 'all_mesh_infos.pkl'), 'wb') as f:
        pickle.dump(rep, f)
    a, b = open_views(ds, 'allview', 'zju_mocap', c), open_views(PreparedDataset(mesh, **kw), 'allview', 'zju_mocap', c)
    for i in (0, 22):
        fa, fb = a.frame(i), b.frame(i)
        for k in ('ray_mask', 'rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'dst_posevec'):
            assert np.array_equal(fa[k], fb[k]), (i, k)
    assert not np.array_equal(a.frame(7)['rays'], b.frame(7)['rays'])


def _dir_bytes(path):
    out = {}
    for base, _, files in os.walk(path):
        for f in files:
            with open(os.path.join(base, f), 'rb') as fh:
                out[os.path.relpath(os.path.join(base, f), path)] = fh.read()
    return out


def test_make_dataset_without_all_cameras_writes_the_directory_it_wrote_before(tmp_path):
    tool = load_tool()
    kw = dict(frames=2, width=48, height=40, seed=5)
    tool.make_dataset(str(tmp_path / 'plain'), **kw)
    tool.make_dataset(str(tmp_path / 'zero'), all_cameras=0, **kw)
    tool.make_dataset(str(tmp_path / 'ring'), all_cameras=3, **kw)
    plain, zero, ring = (_dir_bytes(str(tmp_path / n)) for n in ('plain', 'zero', 'ring'))
    assert sorted(plain) == sorted(zero) == ['cameras.pkl', 'canonical_joints.pkl', 'images/frame_000000.png',
                                             'images/frame_000001.png', 'masks/frame_000000.png', 'masks/frame_000001.png',
                                             'mesh_infos.pkl']
    assert plain == zero
    assert sorted(ring) == sorted(list(plain) + ['all_cameras.pkl']) and all(ring[k] == plain[k] for k in plain)
    rig = pickle.loads(ring['all_cameras.pkl'])
    cams = pickle.loads(ring['cameras.pkl'])
    assert list(rig) == ['frame_000000', 'frame_000001']
    for n in rig:
        assert {k: (v.shape, v.dtype) for k, v in rig[n].items()} == {'intrinsics': ((3, 3, 3), np.float64),
                                                                      'extrinsics': ((3, 4, 4), np.float64)}
        assert np.array_equal(rig[n]['extrinsics'][0], cams[n]['extrinsics'])
        assert np.array_equal(rig[n]['intrinsics'][2], cams[n]['intrinsics'])
        centres = [-E[:3, :3].T.dot(E[:3, 3]) for E in rig[n]['extrinsics']]
        assert min(np.linalg.norm(centres[i] - centres[j]) for i in range(3) for j in range(i)) > 1.0     # a ring, not a point


def test_view_frames_have_the_batch_dimension(golden_dataset):
    import torch
    g, path, ds = golden_dataset
    batches = list(open_views(ds, 'backview', 'zju_mocap', golden_cfg(g)))
    assert len(batches) == 4
    b = batches[2]
    n = int(b['ray_mask'].sum())
    assert b['rays'].shape == (1, 2, n, 3) and b['near'].shape == (1, n, 1) and b['rays'].dtype == torch.float32
    assert b['frame_name'] == ['frame_000002'] and b['img_width'] == 48 and b['img_height'] == 40
    assert b['truth_u8'].shape == (1, 40, 48, 3) and b['truth_u8'].dtype == torch.uint8


def test_recorder_reproduces_the_committed_recording(tmp_path):
    from oracle.ref_harness import shims
    if not os.path.isdir(shims.REF):
        pytest.skip('the reference tree is not on this machine')
    env = {**os.environ, 'OCCNERF_GOLDEN_DIR': str(tmp_path)}
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tools', 'record_view_frames_golden.py')], env=env,
                          stdout=subprocess.DEVNULL, timeout=150)
    new, old = np.load(str(tmp_path / 'view_frames_ref.npz')), golden()
    assert sorted(new.files) == sorted(old)
    for k in old:
        assert new[k].dtype == old[k].dtype and np.array_equal(new[k], old[k]), k
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'freeview_trained_s128.npz'))
    assert os.path.getsize(GOLDEN) < 1 << 20


_LOADER_SCRIPT = '''
import sys
data_type = sys.argv.pop(1)                 # configs parses sys.argv at import
from core.data import create_dataloader
loader = create_dataloader(data_type)
print('LOADER', type(loader).__module__, type(loader).__name__, loader.kind, len(loader), loader.src_type,
      loader.dataset.avg_betas.shape[0])
'''


def _loader(data_type, *opts, cwd=None):
    cmd = [sys.executable, '-c', _LOADER_SCRIPT, data_type, '--cfg',
           os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml')] + list(opts)
    out = subprocess.check_output(cmd, env={**os.environ, 'PYTHONPATH': ROOT}, text=True, timeout=150, cwd=cwd)
    return [line for line in out.splitlines() if line.startswith('LOADER')][0].split()[1:]


def test_create_dataloader_hands_out_the_view_loaders_for_a_dataset_path(golden_dataset, tmp_path):
    g, path, _ = golden_dataset
    opts = ['train.dataset_path', path, 'resize_img_scale', '1.0', 'mweight_volume.volume_size', '4', 'render_frames', '5']
    head = ['occnerf_amd.views', 'ViewFrames']
    assert _loader('freeview', *opts) == head + ['freeview', '5', 'zju_mocap', '10']
    assert _loader('backview', 'freeview.src_type', 'wild', *opts) == head + ['backview', '4', 'wild', '10']
    assert _loader('allview', *opts) == head + ['allview', '23', 'zju_mocap', '10']
    assert _loader('tpose', *opts) == head + ['tpose', '1', 'zju_mocap', '10']
    # the reference's dataset names decide the source type; backview reads the directory movement would
    os.makedirs(str(tmp_path / 'dataset' / 'wild'))
    os.symlink(path, str(tmp_path / 'dataset' / 'wild' / 'someone'))
    named = ['subject', 'someone', 'freeview.dataset', 'monocular_test', 'movement.dataset', 'monocular_test'] + opts[2:]
    assert _loader('freeview', *named, cwd=str(tmp_path)) == head + ['freeview', '5', 'wild', '10']
    assert _loader('backview', *named, cwd=str(tmp_path)) == head + ['backview', '4', 'wild', '10']
    # PreparedDataset's refusals apply unchanged
    with pytest.raises(subprocess.CalledProcessError):
        _loader('freeview', 'train.dataset_path', path, 'resize_img_scale', '0.5')
