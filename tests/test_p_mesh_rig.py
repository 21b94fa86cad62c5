"""GPU: the mesh as a rig.  csrc/mesh_rig.hip against the numpy definition (tests/mesh_rig_restatement.py)
-- joints, counts and flags EQUAL, weights, kept, positions and correctives as bit patterns --, and run.py --type mesh with
mesh_rig.enable end to end: the file it writes, read by tests/gltf_restatement.py, against occnerf_amd.mesh.pose_mesh.  The
bounds are those of tests/test_mesh_rig_restatement.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import gltf_restatement as gr
from tests import mesh_pose_restatement as mp
from tests import mesh_restatement as mr
from tests import mesh_rig_restatement as rig
from tests.gpu_util import DEV, T, build_network, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = (np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32))
SIZES = (1, 63, 64, 65, 257)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _frame_data(idx, dev=DEV):
    fr = mp.synthetic_frame(idx)
    data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev)
            for k in ('dst_Rs', 'dst_Ts', 'dst_posevec', 'cnl_gtfms', 'motion_weights_priors')}
    data.update(cnl_bbox_min_xyz=fr['cnl_bbox_min_xyz'], cnl_bbox_scale_xyz=fr['cnl_bbox_scale_xyz'])
    return data


@pytest.fixture(scope='module')
def seeded():
    """The seeded network (with its non-rigid module, as run.py builds it), the body points and 300 points of the canonical box,
    the device preamble's Rs / Ts of the recorded frames and its volume -- computed once, never changed."""
    net, ctx = build_network(0, False, S=32, non_rigid=True)
    datas = [_frame_data(i) for i in mp.FRAMES]
    pre = [net.render_preamble(d) for d in datas]
    Rs, Ts = torch.stack([p[0] for p in pre]).contiguous(), torch.stack([p[1] for p in pre]).contiguous()
    vol = pre[0][2]
    assert tuple(vol.shape) == (25, 32, 32, 32) and tuple(Rs.shape) == (3, 24, 3, 3)
    assert all(torch.equal(p[2], vol) for p in pre)                          # the volume does not depend on the frame
    bmin, bsc = datas[0]['cnl_bbox_min_xyz'], datas[0]['cnl_bbox_scale_xyz']
    lo = np.asarray(bmin, np.float64)
    box = (lo + np.random.RandomState(12).uniform(-0.05, 1.05, (300, 3)) * 2.0 / np.asarray(bsc, np.float64)).astype(np.float32)
    pts = np.ascontiguousarray(np.concatenate([ctx['point_base'], box]))
    return {'net': net, 'pts': pts, 'datas': datas, 'Rs': Rs, 'Ts': Ts, 'vol': vol, 'vol_np': vol[:24].cpu().numpy(), 'box': (bmin, bsc)}


def _skin(ops, x, vol, bmin, bsc, K):
    out = ops.mesh_skin(T(x), vol if torch.is_tensor(vol) else T(vol), bmin, bsc, K)
    assert [o.dtype for o in out] == [torch.uint8, torch.float32, torch.uint8, torch.float32] and all(o.is_cuda for o in out)
    assert [tuple(o.shape) for o in out] == [(len(x), K), (len(x), K), (len(x),), (len(x),)]
    return [o.cpu().numpy() for o in out]


def _equal(got, want, name, names=('joints', 'weights', 'count', 'kept')):
    for g, w, what in zip(got, want, names):
        same(_bits(g), _bits(w), f'{name}: {what}')


def _hand_cases(K):
    inside = mp.box_points(200, 21, -1.3, 1.3)
    zeros = np.zeros((3, 4, 4, 4), np.float32)
    return {'exactly K': (rig.ladder(K)[0], inside), 'tie at K': (rig.ladder(K + 1, tie=(0, 1))[0], inside),
            'tie among the taken': (rig.ladder(K + 1, tie=(K, K - 1))[0], inside), 'more than K': (rig.ladder(K + 3)[0], inside),
            'no positive bone': (zeros, inside), 'G = 2': (rig.ladder(K + 1, G=2, tie=(0, 1))[0], inside),
            'one bone': (mp.one_bone(4)[2], inside), 'two bones': (mp.two_bones(8)[2], inside), 'two bones, G = 2': (mp.two_bones(2)[2], inside),
            'corner bone': (mp.corner_bone(6)[2], np.concatenate([mp.box_points(200, 3, -1.6, 1.6), mp.box_points(200, 4, 0.5, 1.3)]))}


@pytest.mark.parametrize('K', [4, 8])
def test_skin_is_the_restatement_on_hand_made_volumes(ops, K):
    for name, (vol, x) in _hand_cases(K).items():
        want = rig.skin(x, vol, *BOX, K)
        _equal(_skin(ops, x, vol, *BOX, K), want, f'K {K}, {name}')
        if name == 'tie at K':
            inside = want[2] == K
            assert inside.sum() > 50 and (want[0][inside, K - 1] == 0).all()
        if name == 'corner bone':
            assert set(want[2].tolist()) == {0, 1, 2}


@pytest.mark.parametrize('K', [4, 8])
def test_skin_is_the_restatement_on_the_seeded_checkpoint(ops, seeded, K):
    s = seeded
    want = rig.skin(s['pts'], s['vol_np'], *s['box'], K)
    vol24 = s['vol'][:24]
    got = _skin(ops, s['pts'], vol24, *s['box'], K)
    _equal(got, want, f'K {K}, body and box points')
    assert (want[2][:6890] > 0).all() and (want[2][6890:] == 0).any() and set(want[2].tolist()) >= {0, K}
    again = _skin(ops, s['pts'], vol24, *s['box'], K)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    x = T(s['pts'])
    for V in SIZES:
        part = [o.cpu().numpy() for o in ops.mesh_skin(x[6800:6800 + V].contiguous(), vol24, *s['box'], K)]
        _equal(part, [g[6800:6800 + V] for g in got], f'K {K}, V = {V}')
    out = ops.mesh_skin(x[:0].contiguous(), vol24, *s['box'], K)
    assert [tuple(o.shape) for o in out] == [(0, K), (0, K), (0,), (0,)]
    torch.cuda.synchronize()


@pytest.mark.parametrize('K', [4, 8])
@pytest.mark.parametrize('F', [1, 3])
def test_lbs_is_the_restatement(ops, seeded, K, F):
    """The real Rs / Ts of the frames 0, 3 and 17; the targets are ops.mesh_pose's own positions and flags."""
    s = seeded
    x, vol24 = T(s['pts']), s['vol'][:24]
    joints, weights, _, _ = ops.mesh_skin(x, vol24, *s['box'], K)
    Rs, Ts = s['Rs'][:F].contiguous(), s['Ts'][:F].contiguous()
    posed = ops.mesh_lbs(x, joints, weights, Rs, Ts)
    assert posed.dtype == torch.float32 and tuple(posed.shape) == (F, len(s['pts']), 3)
    args = (s['pts'], joints.cpu().numpy(), weights.cpu().numpy(), Rs.cpu().numpy(), Ts.cpu().numpy())
    same(_bits(posed.cpu().numpy()), _bits(rig.lbs(*args)), f'K {K} F {F}: posed')
    newton = [ops.mesh_pose(x, Rs[f], Ts[f], s['vol'], *s['box']) for f in range(F)]
    target, tflag = torch.stack([n[0] for n in newton]).contiguous(), torch.stack([n[1] for n in newton]).contiguous()
    got = ops.mesh_lbs(x, joints, weights, Rs, Ts, target, tflag, 0.05)
    assert [o.dtype for o in got] == [torch.float32, torch.float32, torch.uint8] and tuple(got[2].shape) == (F, len(s['pts']))
    want = rig.lbs(*args, target.cpu().numpy(), tflag.cpu().numpy(), 0.05)
    _equal([g.cpu().numpy() for g in got], want, f'K {K} F {F}, targets', ('posed', 'delta', 'dflag'))
    assert torch.equal(got[0], posed) and 0 < int(want[2].sum()) < want[2].size
    assert (want[2][tflag.cpu().numpy() != 0] == 1).all() and int((tflag != 0).sum()) > 0         # the box points outside the body
    again = ops.mesh_lbs(x, joints, weights, Rs, Ts, target, tflag, 0.05)
    for a, b in zip(got, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    # a tighter guard flags more, and only changes the flagged
    tight = ops.mesh_lbs(x, joints, weights, Rs, Ts, target, tflag, 0.001)
    _equal([g.cpu().numpy() for g in tight], rig.lbs(*args, target.cpu().numpy(), tflag.cpu().numpy(), 0.001), 'max_delta 1 mm',
           ('posed', 'delta', 'dflag'))
    assert int(tight[2].sum()) > int(got[2].sum())
    for V in SIZES:
        sl = slice(6800, 6800 + V)
        part = ops.mesh_lbs(x[sl].contiguous(), joints[sl].contiguous(), weights[sl].contiguous(), Rs, Ts, target[:, sl].contiguous(),
                            tflag[:, sl].contiguous(), 0.05)
        for a, b, what in zip(part, got, ('posed', 'delta', 'dflag')):
            same(_bits(a.cpu().numpy()), _bits(b[:, sl].cpu().numpy()), f'V = {V}: {what}')
        same(_bits(ops.mesh_lbs(x[sl].contiguous(), joints[sl].contiguous(), weights[sl].contiguous(), Rs, Ts).cpu().numpy()),
             _bits(posed[:, sl].cpu().numpy()), f'V = {V}: posed alone')
    empty = ops.mesh_lbs(x[:0].contiguous(), joints[:0].contiguous(), weights[:0].contiguous(), Rs, Ts)
    assert tuple(empty.shape) == (F, 0, 3)
    torch.cuda.synchronize()


def test_lbs_on_hand_made_rigs(ops):
    # the one-bone volume: the rig's skinning is the start point of mesh_pose, which is its root: equal within tol and one
    # float32 rounding -- the one place where the distance between skinning and the model is asserted: zero by construction
    Rs, Ts, vol, bmin, bsc = mp.one_bone(4)
    x = mp.box_points(300, 1, -0.7, 0.7)
    joints, weights, count, kept = ops.mesh_skin(T(x), T(vol), bmin, bsc, 4)
    posed = ops.mesh_lbs(T(x), joints, weights, T(Rs[None]), T(Ts[None]))
    p, flag, _, _ = ops.mesh_pose(T(x), T(Rs), T(Ts), T(vol), bmin, bsc)
    assert not bool(flag.any())
    gap = np.abs(posed[0].cpu().numpy().astype(np.float64) - p.cpu().numpy().astype(np.float64))
    assert (gap <= 1e-7 + 2.0 ** -24 * np.abs(p.cpu().numpy())).all()
    same(_bits(posed.cpu().numpy()), _bits(rig.lbs(x, joints.cpu().numpy(), weights.cpu().numpy(), Rs[None], Ts[None])), 'one bone')
    # the singular blend, slots of weight 0 with any joint, several frames of random bases
    Rs2 = np.stack([np.eye(3), np.diag([-1.0, -1.0, 1.0])]).astype(np.float32)[None]
    Ts2 = np.zeros((1, 2, 3), np.float32)
    x = mp.box_points(70, 3)
    j = np.tile(np.array([0, 1, 1, 0], np.uint8), (70, 1))
    w = np.tile(np.array([0.5, 0.5, 0.0, 0.0], np.float32), (70, 1))
    target, tf = (x[None] + np.float32(0.01)).astype(np.float32), np.zeros((1, 70), np.uint8)
    got = ops.mesh_lbs(T(x), T(j), T(w), T(Rs2), T(Ts2), T(target), T(tf), 0.05)
    _equal([g.cpu().numpy() for g in got], rig.lbs(x, j, w, Rs2, Ts2, target, tf, 0.05), 'singular', ('posed', 'delta', 'dflag'))
    assert bool(got[2].all()) and not bool(got[1].any())
    Rs3, Ts3 = rig.random_bases(3, 5, 11)
    rng = np.random.RandomState(4)
    j8 = rng.randint(0, 5, (70, 8)).astype(np.uint8)
    w8 = rng.uniform(0, 1, (70, 8)).astype(np.float32)
    w8[rng.uniform(size=w8.shape) < 0.4] = 0.0
    target = (rig.lbs(x, j8, w8, Rs3, Ts3) + rng.uniform(-0.03, 0.03, (3, 70, 3))).astype(np.float32)
    tf = (rng.uniform(size=(3, 70)) < 0.1).astype(np.uint8)
    got = ops.mesh_lbs(T(x), T(j8), T(w8), T(Rs3), T(Ts3), T(target), T(tf), 0.05)
    want = rig.lbs(x, j8, w8, Rs3, Ts3, target, tf, 0.05)
    _equal([g.cpu().numpy() for g in got], want, 'random rigs', ('posed', 'delta', 'dflag'))
    assert 0 < int(want[2].sum()) < want[2].size
    torch.cuda.synchronize()


def test_refusals(ops, seeded):
    s = seeded
    x = T(s['pts'][:10])
    vol24 = s['vol'][:24]
    joints, weights, _, _ = ops.mesh_skin(x, vol24, *s['box'], 4)
    Rs, Ts = s['Rs'], s['Ts']
    with pytest.raises(RuntimeError, match='mesh_skin: K = 5 is neither 4 nor 8'):
        ops.mesh_skin(x, vol24, *s['box'], 5)
    with pytest.raises(RuntimeError, match='mesh_skin: nb = 33 outside 1..32'):
        ops.mesh_skin(x, torch.zeros(33, 4, 4, 4, device=DEV), *s['box'])
    with pytest.raises(RuntimeError, match='mesh_skin: vol must be'):
        ops.mesh_skin(x, torch.zeros(24, 4, 4, 5, device=DEV), *s['box'])
    with pytest.raises(RuntimeError, match='mesh_skin: x_c must be float32 \\[V,3\\]'):
        ops.mesh_skin(x.reshape(-1), vol24, *s['box'])
    with pytest.raises(RuntimeError, match='mesh_lbs: joint index 24 outside \\[0, 24\\)'):
        ops.mesh_lbs(x, torch.full_like(joints, 24), weights, Rs, Ts)
    with pytest.raises(RuntimeError, match='mesh_lbs: joint index 5 outside \\[0, 5\\)'):
        ops.mesh_lbs(x, torch.full_like(joints, 5), weights, Rs[:, :5].contiguous(), Ts[:, :5].contiguous())
    with pytest.raises(RuntimeError, match='mesh_lbs: joints and weights must be'):
        ops.mesh_lbs(x, joints[:, :3].contiguous(), weights[:, :3].contiguous(), Rs, Ts)
    with pytest.raises(RuntimeError, match='mesh_lbs: Rs must be \\[F,nb,3,3\\]'):
        ops.mesh_lbs(x, joints, weights, Rs[0], Ts[0])
    with pytest.raises(RuntimeError, match='mesh_lbs: max_delta = -1.0'):
        ops.mesh_lbs(x, joints, weights, Rs, Ts, torch.zeros(3, 10, 3, device=DEV), torch.zeros(3, 10, device=DEV, dtype=torch.uint8), -1.0)
    with pytest.raises(RuntimeError, match='mesh_lbs: target and target_flag come together'):
        ops.mesh_lbs(x, joints, weights, Rs, Ts, torch.zeros(3, 10, 3, device=DEV))
    with pytest.raises(RuntimeError, match='mesh_lbs: target must be'):
        ops.mesh_lbs(x, joints, weights, Rs, Ts, torch.zeros(2, 10, 3, device=DEV), torch.zeros(3, 10, device=DEV, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='mesh_lbs: joints must be torch.uint8'):
        ops.mesh_lbs(x, joints.int(), weights, Rs, Ts)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ end to end
def _run_py(tmp, *extra):
    cmd = [sys.executable, os.path.join(ROOT, 'run.py'), '--cfg', os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml'),
           '--type', 'mesh', 'mesh.resolution', '32', 'N_samples', '16'] + list(extra)
    os.makedirs(str(tmp), exist_ok=True)
    out = subprocess.run(cmd, cwd=str(tmp), env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return tmp / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'seeded' / 'mesh'


def test_run_py_writes_the_rig(ops, seeded, tmp_path):
    """run.py --type mesh mesh_rig.enable True mesh_rig.frames "[0, 3]" mesh_rig.correctives True on the 32-grid, the level at
    the grid's median density (the seeded weights put no surface at the default level): a surface of random weights all over the
    box, most of whose vertices no bone carries -- nothing below depends on how many.  The file is held against the module:
    its rest pose is mesh.ply, its morph targets are ops.mesh_lbs's correctives, and evaluated at its key times it shows
    mesh.pose_mesh's positions on the vertices the corrective was stored for, within the CPU test's bounds."""
    from occnerf_amd import mesh
    s, net = seeded, seeded['net']
    bmin, bsc = s['box']
    bmax = (np.asarray(bmin, np.float32) + np.float32(2.0) / np.asarray(bsc, np.float32)).astype(np.float32)
    field, _, _ = mesh.density_grid(net, bmin, bmax, 32)
    level = repr(float(field.median().item()))
    folder = _run_py(tmp_path / 'rig', 'mesh.level', level, 'mesh_rig.enable', 'True', 'mesh_rig.frames', '[0, 3]',
                     'mesh_rig.correctives', 'True')
    plain = _run_py(tmp_path / 'plain', 'mesh.level', level)
    # without the keys: the files the code path wrote before, and nothing else
    blob = (folder / 'mesh.ply').read_bytes()
    assert blob == (plain / 'mesh.ply').read_bytes() and sorted(os.listdir(plain)) == ['mesh.json', 'mesh.ply']
    a, b = json.loads((folder / 'mesh.json').read_text()), json.loads((plain / 'mesh.json').read_text())
    assert list(a) == list(b) and a.pop('seconds').keys() == b.pop('seconds').keys() and a == b
    assert sorted(os.listdir(folder)) == ['mesh.json', 'mesh.ply', 'rig.json', 'rigged.glb']
    canon = mr.parse_ply(blob)
    verts = np.ascontiguousarray(np.stack([canon['x'], canon['y'], canon['z']], 1))
    V = verts.shape[0]
    assert V > 500 and canon['faces'].shape[0] > 500
    glb = (folder / 'rigged.glb').read_bytes()
    doc, buf = gr.check_rules(glb)
    prim = doc['meshes'][0]['primitives'][0]
    att = prim['attributes']
    # the rest pose: mesh.ply
    assert gr.accessor(doc, buf, att['POSITION']).tobytes() == verts.tobytes()
    assert np.array_equal(gr.accessor(doc, buf, prim['indices']).reshape(-1, 3), canon['faces'])
    assert np.array_equal(gr.accessor(doc, buf, att['COLOR_0'])[:, :3], np.stack([canon['red'], canon['green'], canon['blue']], 1))
    same(_bits(gr.accessor(doc, buf, att['NORMAL'])), _bits(np.stack([canon['nx'], canon['ny'], canon['nz']], 1)), 'normals')
    # the skin and the correctives: the module's
    x = T(verts)
    joints, weights, count, kept = mesh.skin_mesh(net, x, s['datas'][0], 4)
    same(gr.accessor(doc, buf, att['JOINTS_0']), joints.cpu().numpy(), 'JOINTS_0')
    same(_bits(gr.accessor(doc, buf, att['WEIGHTS_0'])), _bits(weights.cpu().numpy()), 'WEIGHTS_0')
    frames = (0, 3)
    datas = [_frame_data(i) for i in frames]
    newton = [mesh.pose_mesh(net, x, d) for d in datas]
    target, tflag = torch.stack([n[0] for n in newton]).contiguous(), torch.stack([n[1] for n in newton]).contiguous()
    Rs = torch.stack([s['Rs'][0], s['Rs'][1]]).contiguous()
    Ts = torch.stack([s['Ts'][0], s['Ts'][1]]).contiguous()
    assert mp.FRAMES[:2] == frames
    posed, delta, dflag = ops.mesh_lbs(x, joints, weights, Rs, Ts, target, tflag, 0.05)
    assert len(prim['targets']) == 2
    for f in range(2):
        same(_bits(gr.accessor(doc, buf, prim['targets'][f]['POSITION'])), _bits(delta[f].cpu().numpy()), f'morph target {f}')
    # the sidecar: the counts the arrays give
    info = json.loads((folder / 'rig.json').read_text())
    n = count.cpu().numpy()
    assert info['K'] == 4 and info['vertices'] == V and info['influences_histogram'] == np.bincount(n, minlength=5).tolist()
    assert info['bound_to_root_for_want_of_a_bone'] == int((n == 0).sum()) and info['fps'] == 30.0 and info['correctives'] is True
    assert info['joint_names'][0] == 'pelvis' and len(info['joint_parents']) == 24 and 'nothing is rotated' in info['axes']
    assert info['bytes'] == len(glb) and [f['frame'] for f in info['frames']] == [0, 3]
    assert set(info['seconds']) == {'keys', 'skin', 'pose', 'lbs', 'report', 'write'}
    share = kept.cpu().numpy().astype(np.float64)[n > 0]
    assert info['kept_share'] == {'min': float(share.min()), 'mean': float(share.mean()), 'p01': float(np.percentile(share, 1))}
    dist = (posed.double() - target.double()).norm(dim=2).cpu().numpy()
    for f, row in enumerate(info['frames']):
        ok = tflag[f].cpu().numpy() == 0
        assert row['name'] == f'frame_{frames[f]:06d}' and row['corrective_flagged'] == int(dflag[f].sum().item())
        assert row['corrective_stored'] == V - row['corrective_flagged'] and row['corrective_max_m'] == float(delta[f].abs().max().item())
        assert row['lbs_to_model_m'] == {'vertices': int(ok.sum()), 'mean': float(dist[f][ok].mean()),
                                         'p99': float(np.percentile(dist[f][ok], 99)), 'max': float(dist[f][ok].max())}
        assert 0 <= row['translation_minus_rest_offset_max_m'] < 1e-5
    # evaluated at its key times the file shows the model's own posed mesh where a corrective was stored
    t = gr.key_times(doc, buf)
    assert np.array_equal(t, np.array([0.0, np.float32(1.0 / 30.0)], np.float64))
    cnl = mp.synthetic_frame(0)['cnl_gtfms']
    reach = np.linalg.norm(verts[:, None].astype(np.float64) - cnl[None, :, :3, 3].astype(np.float64), axis=2).max() + 0.05
    t_max = max(np.abs(gr.accessor(doc, buf, sm['output'])).max() for sm in doc['animations'][0]['samplers']
                if doc['accessors'][sm['output']]['type'] == 'VEC3')
    _, _, _, p64, M = rig.lbs(verts, joints.cpu().numpy(), weights.cpu().numpy(), Rs.cpu().numpy(), Ts.cpu().numpy(),
                              target.cpu().numpy(), tflag.cpu().numpy(), 0.05, parts=True)
    chain = gr.chain_bound(Rs.cpu().numpy(), reach, np.abs(verts).max() + float(Ts.abs().max().item()),
                           float(t_max), float(posed.abs().max().item()))
    for f in range(2):
        ok = dflag[f].cpu().numpy() == 0
        tgt = target[f].cpu().numpy()
        err = np.linalg.norm(gr.evaluate(doc, buf, t[f]) - tgt.astype(np.float64), axis=1)
        bound = chain + np.sqrt(3.0) * gr.corrective_bound(M[f], delta[f].cpu().numpy(), tgt)
        print(f'\n   key {f}: {int(ok.sum())} of {V} correctives stored; max |file - pose_mesh| = {err[ok].max():.3e} m, bound '
              f'{bound[ok].min():.3e} m')
        assert ok.any() and (err[ok] <= bound[ok]).all()


def test_export_rig_without_correctives(ops, seeded, tmp_path):
    """export_rig itself on 48 body points: the rest pose alone, then three keys at K = 8 under a world node -- the branches the
    run.py test does not take -- and the refusals that need the module."""
    from occnerf_amd import mesh
    s, net = seeded, seeded['net']
    verts = np.ascontiguousarray(s['pts'][np.arange(0, 6890, 144)[:48]])
    kept = {'verts': T(verts), 'faces': np.arange(48, dtype=np.int32).reshape(16, 3),
            'colors': (np.arange(48 * 3) % 251).astype(np.uint8).reshape(48, 3)}
    source = mesh.PoseFrames(None, total_frames=100)
    info = mesh.export_rig(net, str(tmp_path / 'rest'), kept, source, {**mesh.RIG_DEFAULTS, 'enable': True})
    doc, buf = gr.check_rules((tmp_path / 'rest' / 'rigged.glb').read_bytes())
    assert 'animations' not in doc and info['frames'] == [] and info['K'] == 4 and info['influences_histogram'][4] == 48
    assert gr.accessor(doc, buf, doc['meshes'][0]['primitives'][0]['attributes']['POSITION']).tobytes() == verts.tobytes()
    rig8 = {**mesh.RIG_DEFAULTS, 'enable': True, 'frames': list(mp.FRAMES), 'influences': 8, 'world': True, 'fps': 25.0}
    info = mesh.export_rig(net, str(tmp_path / 'keys'), kept, source, rig8)
    again = mesh.export_rig(net, str(tmp_path / 'again'), kept, source, rig8)
    blob = (tmp_path / 'keys' / 'rigged.glb').read_bytes()
    assert blob == (tmp_path / 'again' / 'rigged.glb').read_bytes() and {k: v for k, v in info.items() if k != 'seconds'} == \
        {k: v for k, v in again.items() if k != 'seconds'}
    doc, buf = gr.check_rules(blob)
    att = doc['meshes'][0]['primitives'][0]['attributes']
    assert 'JOINTS_1' in att and 'targets' not in doc['meshes'][0]['primitives'][0] and doc['nodes'][-1]['name'] == 'world'
    assert [f['name'] for f in info['frames']] == [f'frame_{i:06d}' for i in mp.FRAMES] and info['world'] is True
    assert all('corrective_flagged' not in f and f['lbs_to_model_m']['vertices'] == 48 for f in info['frames'])
    joints, weights, _, _ = mesh.skin_mesh(net, kept['verts'], s['datas'][0], 8)
    posed = ops.mesh_lbs(kept['verts'], joints, weights, s['Rs'], s['Ts']).cpu().numpy()
    t = gr.key_times(doc, buf)
    assert np.array_equal(t, (np.arange(3) / 25.0).astype(np.float32).astype(np.float64))
    cnl = mp.synthetic_frame(0)['cnl_gtfms']
    reach = np.linalg.norm(verts[:, None].astype(np.float64) - cnl[None, :, :3, 3].astype(np.float64), axis=2).max()
    t_max = max(np.abs(gr.accessor(doc, buf, sm['output'])).max() for sm in doc['animations'][0]['samplers']
                if doc['accessors'][sm['output']]['type'] == 'VEC3')
    bound = gr.chain_bound(s['Rs'].cpu().numpy(), max(reach, np.sqrt(3.0) * np.abs(posed).max()),
                           np.abs(verts).max() + float(s['Ts'].abs().max().item()), float(t_max), np.sqrt(3.0) * float(np.abs(posed).max()),
                           gr.LONGEST_CHAIN + 1)
    for f in range(3):                                         # the synthetic source stands at the origin: R(Rh) = 1, Th = 0
        err = np.linalg.norm(gr.evaluate(doc, buf, t[f]) - posed[f].astype(np.float64), axis=1)
        print(f'\n   key {f}: max |file - mesh_lbs| = {err.max():.3e} m, bound {bound:.3e} m')
        assert err.max() <= bound
    with pytest.raises(RuntimeError, match='mesh_rig.correctives: 17 frames are more than mesh_rig.max_correctives = 16'):
        mesh.export_rig(net, str(tmp_path / 'no'), kept, source, {**rig8, 'frames': list(range(17)), 'correctives': True})
    with pytest.raises(RuntimeError, match='mesh_rig.frames: frame 100 outside the 100 frames'):
        mesh.export_rig(net, str(tmp_path / 'no'), kept, source, {**rig8, 'frames': [100]})
    with pytest.raises(RuntimeError, match='mesh_rig: the mesh has 0 vertices'):
        mesh.export_rig(net, str(tmp_path / 'no'), {**kept, 'verts': kept['verts'][:0]}, source, rig8)
    with pytest.raises(RuntimeError, match='mesh_rig.influences = 6'):
        mesh.export_rig(net, str(tmp_path / 'no'), kept, source, {**rig8, 'influences': 6})
    assert not (tmp_path / 'no').exists()


def test_one_poser_serves_both_exports(seeded, tmp_path):
    """export_posed then export_rig (K = 8, no correctives) on the 48 body points through one shared mesh.MeshPoser, against the
    same two calls with a poser of their own: the files byte for byte, the sidecars outside their wall times, and every one of
    the three frames solved once, not once per export."""
    from occnerf_amd import mesh
    s, net = seeded, seeded['net']
    verts = np.ascontiguousarray(s['pts'][np.arange(0, 6890, 144)[:48]])
    kept = {'verts': T(verts), 'faces': np.arange(48, dtype=np.int32).reshape(16, 3),
            'colors': (np.arange(48 * 3) % 251).astype(np.uint8).reshape(48, 3)}
    source, frames = mesh.PoseFrames(None, total_frames=100), list(mp.FRAMES)
    rig8 = {**mesh.RIG_DEFAULTS, 'enable': True, 'frames': frames, 'influences': 8}
    poser = mesh.MeshPoser(net, kept['verts'])
    assert poser.solved == 0
    infos = {}
    for name, shared in (('shared', poser), ('own', None)):
        out = str(tmp_path / name)
        infos[name] = (mesh.export_posed(net, out, kept, source, frames, poser=shared),
                       mesh.export_rig(net, out, kept, source, rig8, poser=shared))
        if shared is not None:
            assert poser.solved == 3                      # after export_posed and export_rig: 3, not 6
    assert poser.solved == len(frames) == 3
    files = ['rigged.glb'] + [f'posed/frame_{i:06d}.ply' for i in frames]
    assert sorted(os.listdir(tmp_path / 'shared' / 'posed')) == sorted(os.path.basename(f) for f in files[1:])
    for f in files:
        assert (tmp_path / 'shared' / f).read_bytes() == (tmp_path / 'own' / f).read_bytes(), f

    def timeless(d):
        if isinstance(d, dict):
            return {k: timeless(v) for k, v in d.items() if k != 'seconds'}
        return [timeless(v) for v in d] if isinstance(d, list) else d
    for k, name in enumerate(('posed.json', 'rig.json')):
        a, b = (json.loads((tmp_path / w / name).read_text()) for w in ('shared', 'own'))
        assert timeless(a) == timeless(b) and list(a) == list(b) and len(a['frames']) == 3
        assert timeless(infos['shared'][k]) == timeless(infos['own'][k])
    posed, rigged = (json.loads((tmp_path / 'shared' / name).read_text()) for name in ('posed.json', 'rig.json'))
    assert all(set(f['seconds']) == {'unoffset', 'pose', 'write'} for f in posed['frames'])
    assert set(rigged['seconds']) == {'keys', 'skin', 'pose', 'lbs', 'report', 'write'}
