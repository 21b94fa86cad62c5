"""GPU: the mesh in the pose of a frame.  csrc/mesh_pose.hip against the numpy definition
(tests/mesh_pose_restatement.py) -- positions, flags, step counts and residuals all EQUAL --, the project's own, unchanged warp
as the independent judge of the roots, and occnerf_amd.mesh.pose_mesh / run.py --type mesh with mesh_pose.frames end to end.
The recorded frames, E32 and the bound are those of tests/test_mesh_pose_restatement.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_pose_restatement as mp
from tests import mesh_restatement as mr
from tests.gpu_util import DEV, T, build_network, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-7
NAMES = ('positions', 'flags', 'iters', 'resid')


def _frame_data(idx, dev=DEV):
    fr = mp.synthetic_frame(idx)
    data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev)
            for k in ('dst_Rs', 'dst_Ts', 'dst_posevec', 'cnl_gtfms', 'motion_weights_priors')}
    data.update(cnl_bbox_min_xyz=fr['cnl_bbox_min_xyz'], cnl_bbox_scale_xyz=fr['cnl_bbox_scale_xyz'])
    return data


@pytest.fixture(scope='module')
def seeded():
    """The seeded network, its body points and, per recorded frame, the device preamble's Rs / Ts / vol (numpy, background
    channel dropped) with the restatement's answer on them -- computed once, never changed."""
    net, ctx = build_network(0, False, S=32)
    base = np.ascontiguousarray(ctx['point_base'])
    frames = {}
    for idx in mp.FRAMES:
        data = _frame_data(idx)
        Rs, Ts, vol = net.render_preamble(data)
        args = (Rs.cpu().numpy(), Ts.cpu().numpy(), np.ascontiguousarray(vol.cpu().numpy()[:24]), data['cnl_bbox_min_xyz'],
                data['cnl_bbox_scale_xyz'])
        frames[idx] = {'data': data, 'dev': (Rs, Ts, vol), 'args': args, 'want': mp.pose_points(base, *args)}
    return net, base, frames


def _run(ops, x, Rs, Ts, vol, bmin, bsc, **kw):
    out = ops.mesh_pose(T(x), T(Rs), T(Ts), T(vol), bmin, bsc, **kw)
    assert [o.dtype for o in out] == [torch.float32, torch.uint8, torch.uint8, torch.float32] and all(o.is_cuda for o in out)
    assert tuple(out[0].shape) == (len(x), 3) and all(tuple(o.shape) == (len(x),) for o in out[1:])
    return [o.cpu().numpy() for o in out]


def _equal(got, want, name):
    for g, w, what in zip(got, want, NAMES):
        same(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w,
             f'{name}: {what}')


def _hand_cases():
    near_corner = np.concatenate([mp.box_points(200, 3, -1.6, 1.6), mp.box_points(200, 4, 0.5, 1.3)])
    return {'one bone': (mp.one_bone(4), mp.box_points(300, 1, -0.7, 0.7)),
            'two bones': (mp.two_bones(8), mp.box_points(300, 2)),
            'corner bone': (mp.corner_bone(6), near_corner)}


@pytest.mark.parametrize('name', ['one bone', 'two bones', 'corner bone'])
def test_kernel_is_the_restatement_on_hand_made_volumes(ops, name):
    args, x = _hand_cases()[name]
    want = mp.pose_points(x, *args)
    _equal(_run(ops, x, *args), want, name)
    if name == 'two bones':
        assert want[2].mean() > 1.5 and (want[1] == 0).all()                # Newton steps are taken here, and they end
        short = dict(candidates=1, max_iter=1, tol=1e-12)                    # ... and cut short: flag 1 and the best iterate
        want = mp.pose_points(x, *args, **short)
        assert (want[1] == 1).any()
        _equal(_run(ops, x, *args, **short), want, name + ', cut short')
    if name == 'corner bone':
        assert (want[1] == 2).any() and (want[1] == 0).any()                 # points past the padding: no bone


@pytest.mark.parametrize('idx', mp.FRAMES)
def test_kernel_is_the_restatement_on_the_seeded_checkpoint(ops, seeded, idx):
    net, base, frames = seeded
    f = frames[idx]
    Rs, Ts, vol = f['dev']
    assert tuple(vol.shape) == (25, 32, 32, 32) and tuple(Rs.shape) == (24, 3, 3)
    got = [o.cpu().numpy() for o in ops.mesh_pose(T(base), Rs, Ts, vol, f['args'][3], f['args'][4])]     # 25 channels: 24 are read
    _equal(got, f['want'], f'frame {idx}')
    flagged = float((got[1] != 0).mean())
    print(f'\n   frame {idx}: {flagged:.4f} flagged, {got[2].mean():.2f} Newton steps per point')
    assert flagged <= 0.05


def test_ragged_sizes_and_determinism(ops, seeded):
    net, base, frames = seeded
    f = frames[mp.FRAMES[1]]
    Rs, Ts, vol = f['dev']
    bmin, bsc = f['args'][3], f['args'][4]
    x = T(base)
    full = ops.mesh_pose(x, Rs, Ts, vol, bmin, bsc)
    again = ops.mesh_pose(x, Rs, Ts, vol, bmin, bsc)
    for a, b in zip(full, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    for V in (1, 63, 64, 65, 257):
        for a, b, what in zip(ops.mesh_pose(x[1000:1000 + V].contiguous(), Rs, Ts, vol, bmin, bsc), full, NAMES):
            same(a.cpu().numpy(), b[1000:1000 + V].cpu().numpy(), f'V = {V}: {what}')
    # V = 0: empty tensors, nothing is launched (the null stream is not even looked at)
    out = ops.mesh_pose(x[:0].contiguous(), Rs, Ts, vol, bmin, bsc)
    assert [tuple(o.shape) for o in out] == [(0, 3), (0,), (0,), (0,)]
    assert [o.dtype for o in out] == [torch.float32, torch.uint8, torch.uint8, torch.float32]
    torch.cuda.synchronize()


def _device_warp(ops, p, Rs, Ts, vol, bmin, bsc):
    """The renderer's own sampler and warp at the points p (float32 [n,3] on the device): degenerate rays, S = 1."""
    rays8 = torch.cat([p, torch.zeros(p.shape[0], 5, device=p.device)], 1).contiguous()
    z, x_skel, mask, _ = ops.sample_warp(rays8, 1, torch.zeros(1, device=p.device), Rs, Ts, vol, bmin, bsc)
    return x_skel, mask


@pytest.mark.parametrize('idx', mp.FRAMES)
def test_the_unchanged_warp_maps_the_roots_back(ops, seeded, idx):
    net, base, frames = seeded
    f = frames[idx]
    Rs, Ts, vol = f['dev']
    bmin, bsc = f['args'][3], f['args'][4]
    p, flag, iters, resid = ops.mesh_pose(T(base), Rs, Ts, vol, bmin, bsc)
    x_skel, _ = _device_warp(ops, p, Rs, Ts, vol, bmin, bsc)
    ok = flag.cpu().numpy() == 0
    _, _, J = mp.warp(p.cpu().numpy().astype(np.float64), *f['args'])
    bound = mp.root_bound(p.cpu().numpy(), J, TOL) + mp.E32_CAP
    err = np.abs(x_skel.cpu().numpy().astype(np.float64) - base.astype(np.float64)).max(1)
    print(f'\n   frame {idx}: max |sample_warp(p) - x_c| = {err[ok].max():.3e}, the bound there {bound[ok][np.argmax(err[ok])]:.3e}')
    assert ok.mean() >= 0.95 and (err[ok] <= bound[ok]).all()


@pytest.fixture(scope='module')
def seeded_non_rigid():
    net, ctx = build_network(0, False, S=32, non_rigid=True)
    return net, np.ascontiguousarray(ctx['point_base'])


def test_pose_mesh_with_the_non_rigid_offset(ops, seeded_non_rigid):
    """pose_mesh's points through the frame's warp and its non-rigid offset land on the vertices; the module is left alone."""
    from occnerf_amd import mesh
    from occnerf_amd.modules import hann_window_weights
    net, base = seeded_non_rigid
    idx = mp.FRAMES[2]
    data = _frame_data(idx)
    verts = T(base)
    packed, wconst = net._packed, net._wconst
    stats = {}
    p, flag, iters, resid = mesh.pose_mesh(net, verts, data, stats=stats)
    assert net._packed is packed and set(stats) == {'non_rigid_moving', 'seconds'} and stats['non_rigid_moving'] == 0
    s, moving = net.unoffset_canonical(verts, data)
    assert not bool(moving.any()) and not torch.equal(s, verts)               # the offset is there, and the fixed point ended
    Rs, Ts, vol = net.render_preamble(data)
    bmin, bsc = data['cnl_bbox_min_xyz'], data['cnl_bbox_scale_xyz']
    direct = ops.mesh_pose(s, Rs, Ts, vol, bmin, bsc)
    for a, b in zip((p, flag, iters, resid), direct):
        assert torch.equal(a, b)
    x_skel, _ = _device_warp(ops, p, Rs, Ts, vol, bmin, bsc)
    pk = net._packed_weights()
    nr = net.cfg.non_rigid_motion_mlp
    hann = hann_window_weights(nr.multires, 1e7, nr.kick_in_iter, nr.full_band_iter).tolist()      # as the render forms it
    n = x_skel.shape[0]
    back = ops.nonrigid_rows(x_skel.clone(), torch.arange(n, device=DEV, dtype=torch.int32),
                             torch.full((1,), n, device=DEV, dtype=torch.int32), data['dst_posevec'].reshape(-1),
                             hann, pk.nr_w0, pk.nr_b0, pk.nr)
    ok = flag.cpu().numpy() == 0
    args = (Rs.cpu().numpy(), Ts.cpu().numpy(), vol.cpu().numpy()[:24], bmin, bsc)
    _, _, J = mp.warp(p.cpu().numpy().astype(np.float64), *args)
    bound = mp.root_bound(p.cpu().numpy(), J, TOL) + mp.E32_CAP + 1e-6
    err = np.abs(back.cpu().numpy().astype(np.float64) - base.astype(np.float64)).max(1)
    off = np.abs((s - verts).cpu().numpy()).max()
    print(f'\n   frame {idx}: largest offset undone {off:.3e} m; max |nonrigid(sample_warp(p)) - vertex| = {err[ok].max():.3e}, '
          f'the bound there {bound[ok][np.argmax(err[ok])]:.3e}')
    assert ok.mean() >= 0.95 and (err[ok] <= bound[ok]).all()
    # non_rigid False, or a module that ignores the offsets: the vertices themselves are posed
    plain = mesh.pose_mesh(net, verts, data, non_rigid=False)
    assert torch.equal(plain[0], ops.mesh_pose(verts, Rs, Ts, vol, bmin, bsc)[0])
    net.cfg.ignore_non_rigid_motions = True
    try:
        s2, moving2 = net.unoffset_canonical(verts, data)
        assert torch.equal(s2.view(torch.int32), verts.view(torch.int32)) and not bool(moving2.any()) and s2 is not verts
    finally:
        net.cfg.ignore_non_rigid_motions = False


def test_refusals(ops, seeded):
    net, base, frames = seeded
    f = frames[mp.FRAMES[0]]
    Rs, Ts, vol = f['dev']
    bmin, bsc = f['args'][3], f['args'][4]
    x = T(base[:10])
    with pytest.raises(RuntimeError, match='mesh_pose: candidates = 0 outside 1..8'):
        ops.mesh_pose(x, Rs, Ts, vol, bmin, bsc, candidates=0)
    with pytest.raises(RuntimeError, match='mesh_pose: max_iter = 256 outside 1..255'):
        ops.mesh_pose(x, Rs, Ts, vol, bmin, bsc, max_iter=256)
    with pytest.raises(RuntimeError, match='mesh_pose: x_c must be a CUDA'):
        ops.mesh_pose(x.cpu(), Rs, Ts, vol, bmin, bsc)
    with pytest.raises(RuntimeError, match='mesh_pose: x_c must be torch.float32'):
        ops.mesh_pose(x.double(), Rs, Ts, vol, bmin, bsc)
    with pytest.raises(RuntimeError, match='mesh_pose: x_c must be float32 \\[V,3\\]'):
        ops.mesh_pose(x.reshape(-1), Rs, Ts, vol, bmin, bsc)
    with pytest.raises(RuntimeError, match='mesh_pose: vol must be'):
        ops.mesh_pose(x, Rs, Ts, vol[:23], bmin, bsc)
    with pytest.raises(RuntimeError, match='unoffset_canonical: x_c must be float32 \\[N,3\\]'):
        net.unoffset_canonical(x.double(), f['data'])
    torch.cuda.synchronize()


# ------------------------------------------------------------------ end to end
def _run_py(tmp, *extra):
    cmd = [sys.executable, os.path.join(ROOT, 'run.py'), '--cfg', os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml'),
           '--type', 'mesh', 'mesh.resolution', '24', 'N_samples', '16'] + list(extra)
    os.makedirs(str(tmp), exist_ok=True)
    out = subprocess.run(cmd, cwd=str(tmp), env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return tmp / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'seeded' / 'mesh'


def _face_block(blob):
    head = blob[:blob.index(b'end_header\n') + len(b'end_header\n')].decode('ascii')
    faces = int([l for l in head.splitlines() if l.startswith('element face')][0].split()[-1])
    return blob[len(blob) - faces * 13:]


def test_run_py_poses_a_mesh_with_vertices(seeded_non_rigid, tmp_path):
    """The seeded weights put no surface at the default level (the next test's mesh is empty), so here the level is the median
    of the 24-grid's density, as tools/mesh_export_bench.py takes it: a surface of random weights all over the box.  Most of its
    vertices lie where no bone has a weight -- it is no body, and the 5 % cap does not apply to it -- but every file run.py
    writes can be held against the module: the posed PLY is pose_mesh of mesh.ply's vertices, bit for bit, under mesh.ply's
    faces and colours, with the normals of the posed vertices, and posed.json counts the flags of exactly that call."""
    from occnerf_amd import mesh, synth
    net, _ = seeded_non_rigid
    folder = _run_py(tmp_path, 'mesh.level', '0.7231', 'mesh_pose.frames', '[3]')
    blob = (folder / 'mesh.ply').read_bytes()
    canon = mr.parse_ply(blob)
    verts = np.ascontiguousarray(np.stack([canon['x'], canon['y'], canon['z']], 1))
    V = verts.shape[0]
    assert V > 500 and canon['faces'].shape[0] > 500
    info = json.loads((folder / 'posed.json').read_text())
    assert info['vertices'] == V and len(info['frames']) == 1 and info['non_rigid'] is True and info['world'] is False
    assert (info['candidates'], info['max_iter'], info['tol']) == (3, 20, 1e-7)
    f = info['frames'][0]
    posed_blob = (folder / 'posed' / 'frame_000003.ply').read_bytes()
    assert _face_block(posed_blob) == _face_block(blob) and len(posed_blob) == len(blob)
    ply = mr.parse_ply(posed_blob)
    p, flag, iters, resid = mesh.pose_mesh(net, T(verts), _frame_data(3))
    got = np.stack([ply['x'], ply['y'], ply['z']], 1)
    same(got.view(np.uint32), p.cpu().numpy().view(np.uint32), 'posed vertices')
    for c in ('red', 'green', 'blue'):
        assert np.array_equal(ply[c], canon[c])
    same(np.stack([ply['nx'], ply['ny'], ply['nz']], 1), synth.vertex_normals(got, canon['faces']).astype(np.float32), 'normals')
    counts = np.bincount(flag.cpu().numpy(), minlength=3)
    assert [f['converged'], f['not_converged'], f['no_bone']] == counts.tolist() and f['frame'] == 3
    assert f['worst_resid'] == float(resid.max().item()) and abs(f['mean_iters'] - float(iters.float().mean().item())) < 1e-6
    assert f['flagged_share'] == float(counts[1] + counts[2]) / V and set(f['seconds']) == {'unoffset', 'pose', 'write'}
    print(f"\n   {V} vertices: flags {counts.tolist()}, {f['mean_iters']:.2f} steps per vertex")
    assert counts[0] > 100                           # (the part of the surface that lies in the body is solved)
    # a vertex no bone carries stays where the undone non-rigid offset left it; the others move with their bones
    s, _ = net.unoffset_canonical(T(verts), _frame_data(3))
    none = flag.cpu().numpy() == 2
    assert np.array_equal(got[none], s.cpu().numpy()[none]) and np.abs(got - verts).max() > 0.01


def test_run_py_poses_the_mesh(tmp_path):
    """The command of DESIGN.md section 7i as a user types it.  On the seeded checkpoint the default level leaves no surface
    (tools/mesh_export_bench.py says why), so mesh.ply and the posed PLYs have no vertex: what is checked on them is the files,
    their names, the equal face blocks and that mesh.ply does not depend on the key; the vertices are the test above's."""
    from oracle.chain import per_frame_cpu
    from tests import util
    folder = _run_py(tmp_path / 'posed', 'mesh_pose.frames', '[0, 3]')
    plain = _run_py(tmp_path / 'plain')
    blob = (folder / 'mesh.ply').read_bytes()
    assert blob == (plain / 'mesh.ply').read_bytes() and not (plain / 'posed').exists() and not (plain / 'posed.json').exists()
    canon = mr.parse_ply(blob)
    verts = np.stack([canon['x'], canon['y'], canon['z']], 1)
    V = verts.shape[0]
    info = json.loads((folder / 'posed.json').read_text())
    assert info['vertices'] == V and [f['frame'] for f in info['frames']] == [0, 3] and info['world'] is False
    assert sorted(os.listdir(folder / 'posed')) == ['frame_000000.ply', 'frame_000003.ply']
    ctx = util.model_context(0, False)
    for f in info['frames']:
        posed_blob = (folder / 'posed' / (f['name'] + '.ply')).read_bytes()
        assert _face_block(posed_blob) == _face_block(blob)
        ply = mr.parse_ply(posed_blob)
        assert ply['x'].shape[0] == V and np.array_equal(ply['faces'], canon['faces']) and 'nx' in ply
        for c in ('red', 'green', 'blue'):
            assert np.array_equal(ply[c], canon[c])
        assert f['converged'] + f['not_converged'] + f['no_bone'] == V
        if V:
            # the restatement (on the CPU's per-frame constants, the vertices as they are) stays within the cap on this mesh ...
            fr = mp.synthetic_frame(f['frame'])
            Rs, Ts, vol, _, _ = per_frame_cpu(ctx, fr)
            flag = mp.pose_points(verts, Rs, Ts, vol[:24], fr['cnl_bbox_min_xyz'], fr['cnl_bbox_scale_xyz'])[1]
            print(f"\n   frame {f['frame']}: {V} vertices, restatement flags {float((flag != 0).mean()):.4f}, run.py "
                  f"{f['flagged_share']:.4f}; worst resid {f['worst_resid']:.3e}, {f['mean_iters']:.2f} steps")
            assert float((flag != 0).mean()) <= 0.05
            # ... and so does what run.py wrote
            assert f['flagged_share'] <= 0.05
            assert np.isfinite(np.stack([ply['x'], ply['y'], ply['z']], 1)).all()
