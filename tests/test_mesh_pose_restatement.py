"""CPU: the numpy definition of the posed mesh (tests/mesh_pose_restatement.py) solves what it claims to
solve, and what surrounds the kernel works without a GPU.

Recorded here (and repeated as constants in tests/mesh_pose_restatement.py, which the GPU tests share):
  * E32 = max |CPU oracle's fp32 warp - the restatement's fp64 F| at the posed body points of the seeded checkpoint in frames
    0, 3 and 17 of the synthetic movement sequence: 2.53e-7, 2.99e-7 and 2.90e-7 -> E32 = 2.99e-7, asserted below 4 x that;
  * the restatement leaves 0 of the 6 890 body points flagged in each of the frames 0, 3, 10, 17, 33, 50 and 77 (share 0.0, the
    cap for a recorded frame is 2.5 %); the frames 0, 3 and 17 are the recorded ones, with 2.25, 2.24 and 2.06 Newton steps per
    point on average."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from tests import mesh_pose_restatement as mp
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-7


@functools.lru_cache(maxsize=None)
def _frame(idx):
    """(Rs, Ts, vol[24], bbox_min, bbox_scale, vol[25]) of a recorded frame from the product's per-frame modules on the CPU, and
    the restatement's answer on the seeded checkpoint's body points."""
    from oracle.chain import per_frame_cpu
    ctx = util.model_context(0, False)
    fr = mp.synthetic_frame(idx)
    Rs, Ts, vol, _, _ = per_frame_cpu(ctx, fr)
    args = (Rs, Ts, np.ascontiguousarray(vol[:24]), fr['cnl_bbox_min_xyz'], fr['cnl_bbox_scale_xyz'])
    return args, vol, mp.pose_points(ctx['point_base'], *args), ctx['point_base']


def _oracle_warp32(oracle, p32, Rs, Ts, vol25, bmin, bsc):
    """The CPU oracle's fp32 sampler and warp on the degenerate rays [p, 0, 0, 0, 0, 0], S = 1, t_vals = [0]: the warp at p."""
    z, pts = oracle.sample_rays(mp.degenerate_rays(p32), np.zeros(1, np.float32))
    assert np.array_equal(pts.reshape(-1, 3), np.asarray(p32, np.float32))
    x_skel, mask = oracle.motion_field(pts, Rs, Ts, vol25, bmin, bsc)
    return x_skel.reshape(-1, 3).astype(np.float64), mask.reshape(-1)


def test_one_bone_is_the_rigid_inverse():
    Rs, Ts, vol, bmin, bsc = mp.one_bone(4)
    x = mp.box_points(200, 1, -0.5, 0.5)
    p, flag, iters, resid = mp.pose_points(x, Rs, Ts, vol, bmin, bsc)
    want = np.einsum('ij,ni->nj', Rs[0].astype(np.float64), x.astype(np.float64) - Ts[0].astype(np.float64))
    assert p.dtype == np.float32 and flag.dtype == np.uint8 and iters.dtype == np.uint8 and resid.dtype == np.float32
    assert (flag == 0).all() and iters.max() <= 1
    assert (np.abs(p.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 1e-12).all()
    F, wsum, J = mp.warp(want, Rs, Ts, vol, bmin, bsc)
    assert np.abs(wsum - 1.0).max() < 1e-12 and np.abs(J - Rs[0].astype(np.float64)).max() < 1e-12


def test_jacobian_is_the_derivative_of_F():
    """Central differences of F inside a cell, on the volume where both weight gradients matter."""
    args = mp.two_bones(8)
    p = mp.box_points(64, 5, -0.6, 0.6).astype(np.float64)
    F, wsum, J = mp.warp(p, *args)
    h = 1e-6
    for j in range(3):
        e = np.zeros(3)
        e[j] = h
        num = (mp.warp(p + e, *args, jac=False)[0] - mp.warp(p - e, *args, jac=False)[0]) / (2 * h)
        same_cell = np.all(np.floor(mp.grid_index(p + e, -1.0, 1.0, 8)) == np.floor(mp.grid_index(p - e, -1.0, 1.0, 8)), axis=1)
        assert same_cell.sum() > 50
        assert np.abs(num - J[:, :, j])[same_cell].max() < 1e-6


@pytest.mark.parametrize('idx', mp.FRAMES)
def test_F_against_the_fp32_warp(oracle, idx):
    args, vol25, (p, flag, iters, resid), base = _frame(idx)
    F, wsum, _ = mp.warp(p.astype(np.float64), *args, jac=False)
    got, mask = _oracle_warp32(oracle, p, args[0], args[1], vol25, args[3], args[4])
    e32 = np.abs(got - F).max()
    print(f'\n   frame {idx}: E32 = max |oracle fp32 warp - F64| = {e32:.3e} (recorded {mp.E32:.3e}, cap {mp.E32_CAP:.3e})')
    assert e32 <= mp.E32_CAP


@pytest.mark.parametrize('idx', mp.FRAMES)
def test_roots(oracle, idx):
    args, vol25, (p, flag, iters, resid), base = _frame(idx)
    ok = flag == 0
    F, wsum, J = mp.warp(p.astype(np.float64), *args)
    bound = mp.root_bound(p, J, TOL)
    err = np.abs(F - base.astype(np.float64)).max(1)
    print(f'\n   frame {idx}: max |F64(p32) - x_c| = {err[ok].max():.3e}, the bound there {bound[ok][np.argmax(err[ok])]:.3e}; '
          f'largest resid {resid[ok].max():.3e}')
    assert (err[ok] <= bound[ok]).all()
    assert (resid[ok] <= np.float32(TOL)).all() and (wsum[ok] >= mp.CLAMP * (1 - 1e-6)).all()
    got, _ = _oracle_warp32(oracle, p, args[0], args[1], vol25, args[3], args[4])
    err32 = np.abs(got - base.astype(np.float64)).max(1)
    print(f'   max |oracle fp32 warp(p32) - x_c| = {err32[ok].max():.3e}')
    assert (err32[ok] <= bound[ok] + mp.E32_CAP).all()


@pytest.mark.parametrize('idx', mp.FRAMES)
def test_flagged_share_of_the_recorded_frames(idx):
    _, _, (p, flag, iters, resid), base = _frame(idx)
    share = float((flag != 0).mean())
    print(f'\n   frame {idx}: {int((flag != 0).sum())} of {len(flag)} flagged, {iters.mean():.2f} Newton steps per point')
    assert len(flag) == 6890 and share <= 0.025 and share <= mp.FLAGGED_SHARE[idx] + 1e-12
    assert 0 < iters.mean() < 20


def test_flags_one_and_two():
    args, _, _, base = _frame(mp.FRAMES[0])
    far = (np.asarray(args[3]) - 5.0).reshape(1, 3).astype(np.float32)                   # outside the canonical box
    x = np.concatenate([far, base[:400]])
    p, flag, iters, resid = mp.pose_points(x, *args, candidates=1, max_iter=2)
    assert flag[0] == 2 and iters[0] == 0 and np.array_equal(p[0], x[0])
    F, _, _ = mp.warp(x[:1].astype(np.float64), *args, jac=False)
    assert resid[0] == np.float32(np.abs(F - x[:1]).max())
    # two steps do not solve every point: the unsolved ones carry their best iterate, its residual, and no more than two steps
    one = flag == 1
    assert one.any() and (flag[1:] != 2).all() and iters.max() <= 2
    F, _, _ = mp.warp(p[one].astype(np.float64), *args, jac=False)
    assert np.abs(np.abs(F - x[one]).max(1) - resid[one]).max() < 1e-6
    full = mp.pose_points(x, *args)
    assert (full[1][1:] == 0).all() and (full[2][one] > 2).all()


def test_configuration_and_plumbing():
    from occnerf_amd import mesh
    from occnerf_amd.config import CfgNode, default_cfg
    from occnerf_amd.sequence import SyntheticFrames
    m = default_cfg().mesh_pose
    assert dict(m) == {'frames': None, 'candidates': 3, 'max_iter': 20, 'tol': 1e-7, 'non_rigid': True, 'world': False}
    cfg = default_cfg().merge_from_list(['mesh_pose.frames', '[0, 3]', 'mesh_pose.world', 'True'])
    assert cfg.mesh_pose.frames == [0, 3] and cfg.mesh_pose.world is True and isinstance(cfg.mesh_pose, CfgNode)
    assert default_cfg().merge_from_list(['mesh_pose.frames', 'all']).mesh_pose.frames == 'all'
    src = open(os.path.join(ROOT, 'run.py')).read()
    assert 'export_posed(' in src and "mp.get('frames') is not None" in src and 'keep=kept' in src
    # the synthetic frame source hands over the body constants of the movement sequence run.py renders
    source, ref = mesh.PoseFrames(None, total_frames=100), SyntheticFrames('movement', img_size=8, render_frames=100)
    assert len(source) == 100
    name, data, Rh, Th = source.frame(17)
    want = ref.frame(17)
    assert name == 'frame_000017' and np.array_equal(Rh, np.eye(3)) and not Th.any()
    for k in mesh._POSE_KEYS + ('cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz'):
        assert np.array_equal(data[k], want[k]), k
    # R(Rh) p + Th in float64, rounded once
    rng = np.random.RandomState(3)
    p, Th = rng.randn(50, 3).astype(np.float32), rng.randn(3).astype(np.float32)
    Rh = mp.two_bones()[0][1]
    got = mesh.to_world(p, Rh, Th)
    want = p.astype(np.float64) @ Rh.astype(np.float64).T + Th.astype(np.float64)
    assert got.dtype == np.float32 and (np.abs(got - want) <= 2.0 ** -24 * np.abs(want) + 1e-15).all()
    assert np.array_equal(mesh.to_world(p, np.eye(3), np.zeros(3)), p)
    assert 'posed meshes' not in mesh.__doc__ and 'pose_mesh' in mesh.__doc__


def test_pose_frames_of_a_prepared_dataset(tmp_path):
    """The body constants, names and Rh / Th that dataset.PreparedDataset computes, without opening an image."""
    import importlib.util
    from occnerf_amd import mesh
    from occnerf_amd.dataset import PreparedDataset
    spec = importlib.util.spec_from_file_location('make_synthetic_dataset', os.path.join(ROOT, 'tools', 'make_synthetic_dataset.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    path = str(tmp_path / 'ds')
    tool.make_dataset(path, frames=3, width=32, height=32, seed=0, focal=40.0)
    ds = PreparedDataset(path, device=None)
    source = mesh.PoseFrames(path)
    assert len(source) == len(ds) == 3
    for i in range(3):
        name, data, Rh, Th = source.frame(i)
        want = ds.host_constants(i)
        assert name == ds.frames[i]['frame_name'] and set(data) == set(want)
        for k in want:
            assert np.array_equal(data[k], want[k]) and np.asarray(data[k]).dtype == np.asarray(want[k]).dtype, k
        assert np.array_equal(Rh, ds.frames[i]['Rh']) and np.array_equal(Th, ds.frames[i]['Th'])


def test_c_entry_refuses_bad_arguments_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    from occnerf_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def call(V=5, x=p, Rs=p, nb=24, G=32, candidates=3, max_iter=20, tol=1e-7, out=p):
        return lib.occnerf_mesh_pose(x, V, Rs, p, p, nb, G, p, p, candidates, max_iter, tol, out, p, p, p, None)

    def refused(rc, word):
        msg = lib.occnerf_last_error()
        assert rc != 0 and msg.startswith(b'mesh_pose') and word.encode() in msg, (rc, msg)
    refused(call(Rs=None), 'null')
    refused(call(x=None), 'null')
    refused(call(out=None), 'null')
    refused(call(nb=33), 'nb=33')
    refused(call(nb=0), 'nb=0')
    refused(call(G=1), 'G=1')
    refused(call(candidates=0), 'candidates=0')
    refused(call(candidates=9), 'candidates=9')
    refused(call(max_iter=0), 'max_iter=0')
    refused(call(max_iter=256), 'max_iter=256')
    refused(call(tol=-1.0), 'tol')
    refused(call(tol=float('nan')), 'tol')
    refused(call(V=-1), 'V=-1')
    assert call(V=0, x=None, out=None) == 0              # nothing to do: 0 without a launch (there is no GPU here to launch on)
    assert lib.occnerf_abi_version() == 5


def test_wrappers_refuse_host_tensors_and_the_sources_agree():
    import torch
    from occnerf_amd import ops
    from occnerf_amd.network import Network
    Rs, Ts, vol, bmin, bsc = (torch.from_numpy(a) for a in mp.one_bone())
    with pytest.raises(RuntimeError, match='mesh_pose: x_c must be a CUDA'):
        ops.mesh_pose(torch.zeros(5, 3), Rs, Ts, vol, bmin, bsc)
    with pytest.raises(RuntimeError, match='unoffset_canonical: x_c must be a CUDA'):
        Network.unoffset_canonical(None, torch.zeros(5, 3), {})
    make = open(os.path.join(ROOT, 'occnerf_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\bmesh_pose\.hip\b', make, flags=re.M)
    src = open(os.path.join(ROOT, 'occnerf_amd', 'csrc', 'mesh_pose.hip')).read()
    assert 'fma' not in re.sub(r'//[^\n]*', '', src).lower() and 'atomic' not in re.sub(r'//[^\n]*', '', src).lower()
    assert 'kPoseClamp = 1e-4' in src and mp.CLAMP == 1e-4


@pytest.mark.parametrize('key', ['mesh_pose.frames', 'mesh_view.frames'])
def test_frame_indices_are_one_rule_under_every_key(key):
    """mesh._frame_indices serves export_posed, export_rig and mesh_view.export_views: the same list and the same refusal,
    named after the key that asked."""
    from occnerf_amd import mesh
    source = mesh.PoseFrames(None, total_frames=7)
    assert mesh._frame_indices(source, 'all', key) == list(range(7))
    assert mesh._frame_indices(source, [6, 0, 3, 3], key) == [6, 0, 3, 3]
    assert mesh._frame_indices(source, (np.int64(2), 5.0), key) == [2, 5] and mesh._frame_indices(source, [], key) == []
    for bad in ([0, 7], [-1], [3, 100]):
        with pytest.raises(RuntimeError, match=f'^{re.escape(key)}: frame {bad[-1]} outside the 7 frames of the source$'):
            mesh._frame_indices(source, bad, key)


def test_export_views_refuses_a_frame_through_the_shared_rule():
    """mesh_view.export_views takes its frame list from mesh._frame_indices: the refusal is that function's, before anything is
    posed or written (a network that is only a device and a source that is only a length get that far)."""
    import types

    import torch
    from occnerf_amd import mesh_view
    net = types.SimpleNamespace(point_base=torch.zeros(1))
    with pytest.raises(RuntimeError, match='^mesh_view.frames: frame 7 outside the 7 frames of the source$'):
        mesh_view.export_views(net, os.devnull, {}, range(7), [0, 7])


def test_shared_mesh_header_keeps_the_kernels_rules():
    """What mesh_raster.hip, mesh_texture.hip and mesh_normal.hip share lives in mesh_screen.h and mesh_atlas.h: neither holds a
    fused multiply-add or an atomic of its own, and every object file is rebuilt when one changes."""
    make = open(os.path.join(ROOT, 'occnerf_amd', 'csrc', 'Makefile')).read()
    rule = re.search(r'^build/%\.o:.*$', make, flags=re.M).group(0)
    for header in ('mesh_screen.h', 'mesh_atlas.h'):
        src = re.sub(r'//[^\n]*', '', open(os.path.join(ROOT, 'occnerf_amd', 'csrc', header)).read()).lower()
        assert 'fma' not in src and 'atomic' not in src and re.search(rf'\b{re.escape(header)}\b', rule), header
