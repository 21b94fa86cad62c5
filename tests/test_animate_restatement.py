"""CPU: the host side of run.py --type animate (occnerf_amd/animate.py) and the definition of the skeleton panel
(tests/skeleton_restatement.py), on tool-made datasets of 5 frames of 96 x 80, seeds 0 and 1.

The tool's camera turns a quarter orbit over a sequence, and an animate sequence is shot by ONE camera, the source frame's;
the identity test therefore takes every frame in turn as the source frame and compares that frame's K and E with the
movement loader's: no frame's camera is left unchecked."""
import os

import numpy as np
import pytest

from occnerf_amd import animate as A
from occnerf_amd import synth
from occnerf_amd.dataset import PreparedDataset, apply_global_tfm_to_camera
from occnerf_amd.views import ViewFrames
from tests import animate_cases as cases
from tests import skeleton_restatement as S

BBOX_OFFSET = 0.3


def same_bytes(got, want, name):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    assert got.tobytes() == want.tobytes(), f'{name}: {int((got != want).sum())} of {got.size} entries differ'


@pytest.fixture(scope='module')
def data(tmp_path_factory):
    paths = cases.make_datasets(tmp_path_factory.mktemp('animate'))
    subject = PreparedDataset(paths[0], device=None, volume_size=4, bbox_offset=BBOX_OFFSET)
    return {'paths': paths, 'subject': subject, 'own': A.read_motion(paths[0]), 'other': A.read_motion(paths[1])}


def source(data, motion, **kw):
    return A.AnimateFrames(data['subject'], data[motion], bbox_offset=BBOX_OFFSET, **kw)


# ------------------------------------------------------------------ identity
def test_the_subjects_own_motion_gives_the_movement_loaders_frames(data):
    ds = data['subject']
    worst = 0.0
    for src in range(len(ds)):
        frames = source(data, 'own', frame_idx=src, align=False, substeps=1, camera='fixed')
        assert len(frames) == len(ds) == 5
        for t in range(len(ds)):
            got, want = frames.frame(t), ds.host_constants(t)
            for k in ('dst_Rs', 'dst_Ts', 'dst_posevec', 'cnl_gtfms', 'motion_weights_priors', 'cnl_bbox_min_xyz',
                      'cnl_bbox_max_xyz', 'cnl_bbox_scale_xyz'):
                same_bytes(got[k], want[k], f'source {src} frame {t}: {k}')
            assert 'truth_u8' not in got
            # the box: forward kinematics of the float32 tpose_joints against the pickle's joints, rounded once from float64:
            # at most 9 links of one float32 ulp of a sub-metre offset (6e-8) each, plus the final rounding (1.2e-7)
            v = frames.view(t)
            for k, w in (('min', 'dst_bbox_min'), ('max', 'dst_bbox_max')):
                worst = max(worst, float(np.abs(np.asarray(v[k], np.float64) - ds.frames[t][w]).max()))
        v = frames.view(src)                               # the source frame's camera is the one calibrated camera of the run
        same_bytes(v['K'], ds.frames[src]['K'], f'frame {src}: K')
        same_bytes(v['E'], ds.frames[src]['E'], f'frame {src}: E')
    print(f'\n   box against the movement loader: max |diff| = {worst:.3e} m')
    assert worst <= 1e-6


def test_host_frames_carry_what_the_renderer_takes(data):
    frames = source(data, 'own', align=False)
    batches = list(frames)
    assert len(batches) == 5
    for k in ('rays', 'near', 'far', 'ray_mask', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec',
              'cnl_bbox_min_xyz', 'cnl_bbox_max_xyz', 'cnl_bbox_scale_xyz', 'bgcolor', 'img_width', 'img_height', 'frame_name',
              'camera_K', 'camera_E'):
        assert k in batches[0], k
    assert batches[0]['rays'].shape[0] == 1 and batches[0]['rays'].shape[1] == 2 and batches[0]['rays'].shape[2] > 100
    assert batches[3]['frame_name'] == ['animate_000003'] and 'truth_u8' not in batches[0]


# ------------------------------------------------------------------ retargeting
def test_another_captures_motion_on_the_subject(data):
    frames = source(data, 'other')
    other, ds = data['other'], data['subject']
    same_bytes(frames.poses, other['poses'], 'poses are the motion\'s')
    assert not np.array_equal(other['poses'], data['own']['poses'])
    for t in range(len(frames)):
        v = frames.view(t)
        same_bytes(v['dst_Ts'], ds.frames[0]['dst_Ts'], f'frame {t}: dst_Ts are the subject\'s')
        same_bytes(v['dst_posevec'], other['poses'][t, 3:] + 1e-2, f'frame {t}: dst_posevec')
        joints = synth.posed_joints(other['poses'][t], ds.canonical_joints)
        same_bytes(v['joints'], joints, f'frame {t}: joints')
        assert (joints - BBOX_OFFSET >= v['min'] - 1e-6).all() and (joints + BBOX_OFFSET <= v['max'] + 1e-6).all()
        assert (joints > v['min']).all() and (joints < v['max']).all()


# ------------------------------------------------------------------ resampling
def rel_angle(a, b):
    """The angle of R(a)^T R(b) for axis-angle rows, float64, by atan2 of the quaternion's parts."""
    qa, qb = A.quat_of_axis_angle(a), A.quat_of_axis_angle(b)
    w = (qa * qb).sum(-1)
    x = qa[..., :1] * qb[..., 1:] - qb[..., :1] * qa[..., 1:] - np.cross(qa[..., 1:], qb[..., 1:])
    return 2.0 * np.arctan2(np.sqrt((x * x).sum(-1)), np.abs(w))


def seeded_motion(T=4, seed=5):
    rng = np.random.RandomState(seed)
    poses = (rng.randn(T, 72) * 0.4).astype(np.float32)
    poses[:, :3] = 0                                       # the root pose of every prepared dataset
    poses[:, 12:15] = poses[0, 12:15]                      # joint 4 never moves
    poses[1, 30:33] = (np.float32(3.0) * poses[1, 30:33] / np.linalg.norm(poses[1, 30:33])).astype(np.float32)     # a wide turn
    Rh = (rng.randn(T, 3) * 0.5).astype(np.float32)
    Th = rng.randn(T, 3).astype(np.float32)
    return poses, Rh, Th


def test_substeps_one_is_the_motion_itself():
    poses, Rh, Th = seeded_motion()
    p, r, t, key, u = A.resample_motion(poses, Rh, Th, 1)
    same_bytes(p, poses, 'poses')
    same_bytes(r, Rh, 'Rh')
    same_bytes(t, Th, 'Th')
    assert key.tolist() == [[0, 1], [1, 2], [2, 3], [3, 3]] and (u == 0).all()


@pytest.mark.parametrize('n', [2, 3, 4])
def test_resampling_properties(n):
    poses, Rh, Th = seeded_motion()
    T = poses.shape[0]
    p, r, t, key, u = A.resample_motion(poses, Rh, Th, n)
    assert p.shape == ((T - 1) * n + 1, 72) and r.shape == t.shape == ((T - 1) * n + 1, 3)
    assert p.dtype == r.dtype == t.dtype == np.float32
    assert np.isfinite(p).all() and np.isfinite(r).all() and np.isfinite(t).all()          # zero rotations included
    same_bytes(p[::n], poses, 'keyframes are copied: poses')
    same_bytes(r[::n], Rh, 'keyframes are copied: Rh')
    same_bytes(t[::n], Th, 'keyframes are copied: Th')
    assert key[:, 0].tolist() == [i // n for i in range(len(p))] and np.allclose(u, [(i % n) / n for i in range(len(p))])
    for i in range(len(p)):                                # identical keyframes: identical bytes in between
        same_bytes(p[i, :3], poses[0, :3], f'frame {i}: the zero root')
        same_bytes(p[i, 12:15], poses[0, 12:15], f'frame {i}: the joint that never moves')
    # the n steps of an interval turn by equal angles, and they add up to the interval's own (the shorter arc)
    rot = np.concatenate([p.reshape(-1, 24, 3), r[:, None]], 1)
    steps = rel_angle(rot[:-1], rot[1:]).reshape(T - 1, n, 25)
    whole = rel_angle(rot[:-n:n], rot[n::n])
    worst = float(np.abs(steps - steps.mean(1, keepdims=True)).max())
    print(f'\n   n = {n}: steps differ from their mean by at most {worst:.3e} rad')
    assert worst <= 1e-6
    assert np.abs(steps.sum(1) - whole).max() <= 1e-5 and (whole <= np.pi + 1e-9).all() and whole.max() > 2.0
    # Th is linear
    lin = Th[:-1, None].astype(np.float64) + (np.arange(n) / n)[None, :, None] * (Th[1:, None].astype(np.float64) - Th[:-1, None])
    assert np.abs(t[:-1].reshape(T - 1, n, 3) - lin).max() <= 1e-6


def test_q_and_minus_q_are_the_same_rotation():
    rng = np.random.RandomState(2)
    q0, q1 = rng.randn(50, 4), rng.randn(50, 4)
    q0, q1 = q0 / np.linalg.norm(q0, axis=1, keepdims=True), q1 / np.linalg.norm(q1, axis=1, keepdims=True)
    u = np.float64(0.3)
    a = A.axis_angle_of_quat(A.slerp(q0, q1, u))
    for b in (A.slerp(q0, -q1, u), A.slerp(-q0, q1, u), A.slerp(-q0, -q1, u)):
        assert np.abs(a - A.axis_angle_of_quat(b)).max() <= 1e-12
    assert np.abs(A.axis_angle_of_quat(q0) - A.axis_angle_of_quat(-q0)).max() == 0.0
    # the round trip, and the matrix route, agree with rodrigues_exact
    v = rng.randn(20, 3)
    assert np.abs(A.axis_angle_of_quat(A.quat_of_axis_angle(v)) - v).max() <= 1e-12
    R = np.stack([synth.rodrigues_exact(x) for x in v])
    assert np.abs(A.axis_angle_of_matrix(R) - v).max() <= 1e-12
    assert np.array_equal(A.quat_of_axis_angle(np.zeros(3)), [1., 0., 0., 0.])
    assert np.array_equal(A.axis_angle_of_quat(np.array([1., 0., 0., 0.])), np.zeros(3))


# ------------------------------------------------------------------ alignment and cameras
def test_align_puts_frame_zero_on_the_source_frame(data):
    ds = data['subject']
    for src in (0, 3):
        frames = source(data, 'other', frame_idx=src, align=True)
        f = ds.frames[src]
        assert np.abs(frames.Rh[0] - f['Rh_vec']).max() <= 4 * np.finfo(np.float32).eps
        same_bytes(frames.Th[0], f['Th'], 'Th of frame 0')
        # ... and is one rigid map: the motion's own frame-to-frame turns and steps are kept
        other = data['other']
        R = [synth.rodrigues_exact(r) for r in other['Rh']]
        Rn = [synth.rodrigues_exact(r) for r in frames.Rh]
        M = synth.rodrigues_exact(f['Rh_vec']).dot(R[0].T)
        for t in range(1, 5):
            assert np.abs(Rn[0].T.dot(Rn[t]) - R[0].T.dot(R[t])).max() <= 1e-6
            assert np.abs((frames.Th[t] - frames.Th[0]) - M.dot(other['Th'][t].astype(np.float64) - other['Th'][0])).max() <= 1e-6
    raw = source(data, 'other', align=False)
    same_bytes(raw.Rh, data['other']['Rh'], 'align False: Rh as it is')
    same_bytes(raw.Th, data['other']['Th'], 'align False: Th as it is')


def test_follow_and_fixed_cameras(data):
    ds = data['subject']
    f = ds.frames[2]
    follow = source(data, 'other', frame_idx=2, camera='follow')
    fixed = source(data, 'other', frame_idx=2, camera='fixed')
    for t in range(5):
        same_bytes(follow.view(t)['E'], apply_global_tfm_to_camera(f['extrinsics'], follow.Rh[t], f['Th']), f'follow {t}')
        same_bytes(fixed.view(t)['E'], apply_global_tfm_to_camera(f['extrinsics'], fixed.Rh[t], fixed.Th[t]), f'fixed {t}')
        same_bytes(follow.view(t)['K'], f['K'], f'follow {t}: K')
    assert not np.array_equal(follow.view(4)['E'], fixed.view(4)['E'])


def test_orbit_is_freeviews_camera(data):
    ds, n = data['subject'], 6
    own = data['own']
    still = dict(own, poses=np.repeat(own['poses'][1:2], n, 0), Rh=np.repeat(own['Rh'][1:2], n, 0),
                 Th=np.repeat(own['Th'][1:2], n, 0))
    for src_type in ('zju_mocap', 'wild'):
        frames = A.AnimateFrames(ds, still, frame_idx=1, align=False, camera='orbit', src_type=src_type, render_frames=n,
                                 bbox_offset=BBOX_OFFSET)
        free = ViewFrames(ds, 'freeview', src_type=src_type, render_frames=n, frame_idx=1)
        assert len(frames) == len(free) == n
        for t in range(n):
            same_bytes(frames.view(t)['K'], free.view(t)['K'], f'{src_type} {t}: K')
            same_bytes(frames.view(t)['E'], free.view(t)['E'], f'{src_type} {t}: E')
        assert not np.array_equal(frames.view(1)['E'], frames.view(0)['E'])


# ------------------------------------------------------------------ npz motions and refusals
def test_npz_motions(data, tmp_path):
    own = data['own']
    full = own['poses'].copy()
    full[:, :3] = own['Rh']                                # a mocap clip: the root rotation inside poses, no Rh, no Th
    np.savez(tmp_path / 'clip.npz', poses=full.reshape(-1, 24, 3))
    m = A.read_motion(str(tmp_path / 'clip.npz'))
    same_bytes(m['Rh'], own['Rh'], 'Rh split from poses')
    same_bytes(m['poses'], own['poses'], 'poses with the root zeroed')
    assert m['Th'] is None and m['kind'] == 'npz'
    frames = source({**data, 'clip': m}, 'clip', frame_idx=2, align=False)
    for t in range(5):
        same_bytes(frames.Th[t], data['subject'].frames[2]['Th'], f'frame {t}: the source frame\'s Th')
    np.savez(tmp_path / 'whole.npz', poses=own['poses'].astype(np.float64), Rh=own['Rh'], Th=own['Th'])
    m = A.read_motion(str(tmp_path / 'whole.npz'))
    for k in ('poses', 'Rh', 'Th'):
        same_bytes(m[k], own[k], k)


def test_refusals_are_made_by_name(data, tmp_path):
    own = data['own']
    with pytest.raises(FileNotFoundError, match="animate.motion '.*nowhere' does not exist"):
        A.read_motion(str(tmp_path / 'nowhere'))
    os.makedirs(tmp_path / 'empty_dir')
    with pytest.raises(FileNotFoundError, match='no mesh_infos.pkl'):
        A.read_motion(str(tmp_path / 'empty_dir'))
    (tmp_path / 'motion.txt').write_text('x')
    with pytest.raises(ValueError, match='neither a directory nor an .npz'):
        A.read_motion(str(tmp_path / 'motion.txt'))

    def npz(**arrays):
        np.savez(tmp_path / 'bad.npz', **arrays)
        return str(tmp_path / 'bad.npz')

    with pytest.raises(KeyError, match="no 'poses'"):
        A.read_motion(npz(Rh=own['Rh']))
    with pytest.raises(ValueError, match=r"'poses' has shape \(5, 71\)"):
        A.read_motion(npz(poses=own['poses'][:, :71]))
    with pytest.raises(ValueError, match=r"'Rh' has shape \(4, 3\)"):
        A.read_motion(npz(poses=own['poses'], Rh=own['Rh'][:4]))
    with pytest.raises(ValueError, match=r"'Th' has shape \(5, 2\)"):
        A.read_motion(npz(poses=own['poses'], Th=own['Th'][:, :2]))
    with pytest.raises(TypeError, match="'poses' cannot be cast to float"):
        A.read_motion(npz(poses=np.full((5, 72), 'a')))
    bad = own['poses'].copy()
    bad[2, 7] = np.nan
    with pytest.raises(ValueError, match="'poses' holds non-finite values"):
        A.read_motion(npz(poses=bad))
    bad = own['Th'].copy()
    bad[0, 0] = np.inf
    with pytest.raises(ValueError, match="'Th' holds non-finite values"):
        A.read_motion(npz(poses=own['poses'], Th=bad))
    with pytest.raises(ValueError, match=r'no frame \(T == 0\)'):
        A.read_motion(npz(poses=np.zeros((0, 72), np.float32)))
    with pytest.raises(ValueError, match='animate.substeps = 0'):
        source(data, 'own', substeps=0)
    with pytest.raises(ValueError, match='animate.substeps = 0'):
        A.resample_motion(own['poses'], own['Rh'], own['Th'], 0)
    for idx in (-1, 5):
        with pytest.raises(IndexError, match=f'animate.frame_idx {idx}: .* has 5 frames'):
            source(data, 'own', frame_idx=idx)
    with pytest.raises(ValueError, match="animate.camera 'dolly'"):
        source(data, 'own', camera='dolly')


_LOADER_SCRIPT = '''
import sys
sys.argv = [sys.argv[0], '--cfg', sys.argv[1]] + sys.argv[2:]
from core.data import create_dataloader
loader = create_dataloader('animate')
print('LOADER', type(loader).__name__, len(loader), loader.camera, loader.substeps, loader.align)
'''


def test_create_dataloader_knows_the_type(data):
    """The data entry point hands out the loader for a prepared dataset, with the configured keys, and refuses the synthetic
    frame source and a missing motion by name -- before a GPU is touched: this runs without one."""
    import subprocess
    import sys
    cfg = os.path.join(cases.ROOT, 'configs/occnerf/synthetic/occnerf.yaml')
    base = [sys.executable, '-c', _LOADER_SCRIPT, cfg]
    env = {**os.environ, 'PYTHONPATH': cases.ROOT}
    opts = ['train.dataset_path', data['paths'][0], 'resize_img_scale', '1.0', 'mweight_volume.volume_size', '4']
    out = subprocess.run(base + opts + ['animate.motion', data['paths'][1], 'animate.substeps', '3', 'animate.camera', 'follow'],
                         env=env, capture_output=True, text=True, timeout=150)
    assert out.returncode == 0, out.stderr[-2000:]
    assert [ln for ln in out.stdout.splitlines() if ln.startswith('LOADER')] == ['LOADER AnimateFrames 13 follow 3 True']
    out = subprocess.run(base + ['animate.motion', data['paths'][1]], env=env, capture_output=True, text=True, timeout=150)
    assert out.returncode != 0 and 'the synthetic frame source has' in out.stderr, out.stderr[-1500:]
    # what from_cfg refuses before it opens the subject, on a configuration node built in this process
    from occnerf_amd.config import default_cfg
    for keys, error, word in (({}, ValueError, 'animate.motion PATH'),
                              ({'motion': data['paths'][1] + '_missing'}, FileNotFoundError, 'does not exist'),
                              ({'motion': data['paths'][1], 'substeps': 0}, ValueError, 'animate.substeps = 0'),
                              ({'motion': data['paths'][1], 'camera': 'dolly'}, ValueError, "animate.camera 'dolly'")):
        cfg = default_cfg()
        cfg.animate.update(keys)
        with pytest.raises(error, match=word):
            A.AnimateFrames.from_cfg(cfg, os.path.join(data['paths'][0], 'not_opened'))


# ------------------------------------------------------------------ the skeleton panel's definition
_panels = {}


def panel(name, size=(cases.W, cases.H)):
    key = (name, size)
    if key not in _panels:
        _panels[key] = S.skeleton_panel(**cases.definition_args(cases.all_cases()[name], *size))
    return _panels[key]


@pytest.mark.parametrize('name', sorted(cases.hand_cases()))
def test_hand_cases_show_what_they_are_there_for(name):
    case, got = cases.hand_cases()[name], panel(name)
    bones = set(np.unique(got['winner'][(got['winner'] >= 0) & (got['winner'] < S.BONES)]).tolist())
    assert len(bones) >= 2, bones                          # at least two bones cover pixels
    assert got['n_cover'].max() >= 2                       # somewhere two primitives overlap: the depth rule decides
    assert got['dropped'] == case['dropped'] and got['covered'] == int((got['winner'] >= 0).sum()) > 0
    assert (got['img'][got['winner'] < 0] == cases.BG).all()
    prims, _ = S.primitives(case['joints'], case['K'], case['E'], cases.BONE_PX)
    for q in bones:                                        # a bone that shows has both its ends
        assert prims[q]['ok']
    for q, p in enumerate(prims[:S.BONES]):                # a dropped joint removes its bones
        a = q + 1
        assert p['ok'] == bool(case['joints'][a, 2] > 0 and case['joints'][S.PARENT[a], 2] > 0
                               and np.isfinite(case['joints'][[a, S.PARENT[a]]]).all())
    if 'cross' in case:
        (j, i), want = case['cross']
        assert got['n_cover'][i, j] == 2 and got['winner'][i, j] == want, (got['n_cover'][i, j], got['winner'][i, j], want)
        same_bytes(got['img'][i, j], cases.PALETTE[want + 1], 'the crossing shows the winner\'s colour')
    if name == 'off_screen':
        assert cases.BONE_OF[18] not in bones and prims[cases.BONE_OF[18]]['ok']
        wide = S.skeleton_panel(**cases.definition_args(case, 330, 330))
        assert (wide['winner'] == cases.BONE_OF[18]).any()          # it is there, beyond the border
    if name == 'border':
        w = got['winner'] == cases.BONE_OF[19]
        assert w[0].any() and w.any(0)[-1]                 # it reaches the top row and the last column
    if name == 'behind':
        assert not prims[cases.BONE_OF[7]]['ok'] and not prims[cases.BONE_OF[10]]['ok'] and prims[S.BONES + 10]['ok']
        assert (got['winner'] == S.BONES + 10).any()
    if name == 'zero_length':
        p = prims[cases.BONE_OF[8]]
        assert p['ok'] and p['l2'] == 0.0 and not prims[S.BONES + 11]['ok'] and not prims[cases.BONE_OF[11]]['ok']


def test_the_definition_is_deterministic_and_crops():
    for name in ('generic', 'cross_equal', 'all_dropped'):
        case = cases.all_cases()[name]
        first, again = panel(name), S.skeleton_panel(**cases.definition_args(case))
        for k in ('img', 'winner', 'n_cover'):
            same_bytes(again[k], first[k], f'{name}: second run {k}')
        for w, h in cases.SIZES:                           # a smaller image is a crop: the camera stays
            same_bytes(panel(name, (w, h))['img'], first['img'][:h, :w], f'{name}: {w} x {h}')
    generic = panel('generic')
    assert generic['dropped'] == 0 and len(np.unique(generic['winner'])) > 30 and generic['n_cover'].max() >= 3
    empty = panel('all_dropped')
    assert empty['dropped'] == 24 and empty['covered'] == 0 and (empty['img'] == cases.BG).all()
    with pytest.raises(NotImplementedError, match='skew'):
        S.skeleton_panel(**{**cases.definition_args(cases.generic_case()), 'K': np.array([[1., .1, 0.], [0., 1., 0.], [0., 0., 1.]])})
