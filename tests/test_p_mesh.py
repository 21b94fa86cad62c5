"""GPU: the mesh export.  csrc/mesh.hip's three kernels against the numpy definition
(tests/mesh_restatement.py) -- row counts, triangle keys, welded faces and float32 positions all EQUAL --,
Network.query_canonical against the CPU oracle's chain with test_a_rows.py's bars, and occnerf_amd.mesh / run.py --type mesh
end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_restatement as mr
from tests import util
from tests.gpu_util import DEV, T, build_network, same, stagewise_table

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BBOX_MIN, H = np.array([-1.25, 0.5, 2.0]), 0.037


def _device_keys(ops, field, level):
    row_count = ops.mesh_count(field, level)
    ends = torch.cumsum(row_count, 0, dtype=torch.int64)
    total = int(ends[-1].item())
    return row_count, (ends - row_count).contiguous(), total


def _check_against_restatement(ops, f, level, name):
    from occnerf_amd import mesh
    want_count, want_keys = mr.extract_keys(f, level)
    fd = T(f)
    row_count, row_start, total = _device_keys(ops, fd, level)
    same(row_count.cpu().numpy(), want_count, f'{name}: row_count')
    assert total == want_keys.shape[0]
    tri_keys = ops.mesh_emit(fd, level, row_start, total)
    same(tri_keys.cpu().numpy(), want_keys, f'{name}: tri_keys')
    want_vkeys, want_faces = mr.weld(want_keys)
    want_pos = mr.vertices(want_vkeys, f, level, BBOX_MIN, H)
    if total:
        vkeys, inverse = torch.unique(tri_keys, sorted=True, return_inverse=True)
        same(vkeys.cpu().numpy(), want_vkeys, f'{name}: welded keys')
        same(inverse.reshape(-1, 3).to(torch.int32).cpu().numpy(), want_faces, f'{name}: faces')
        pos = ops.mesh_vertices(vkeys, fd, level, BBOX_MIN, H)
        assert pos.dtype == torch.float32
        same(pos.cpu().numpy(), want_pos, f'{name}: positions')
    verts, faces = mesh.extract_mesh(fd, level, BBOX_MIN, H)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and verts.is_cuda and faces.is_cuda
    same(verts.cpu().numpy(), want_pos, f'{name}: extract_mesh positions')
    same(faces.cpu().numpy(), want_faces, f'{name}: extract_mesh faces')
    return total


def test_kernels_on_the_random_grids(ops):
    total = sum(_check_against_restatement(ops, f, 0.0, f'random field {i}') for i, f in enumerate(mr.random_fields()))
    assert total > 1000


@pytest.mark.parametrize('name', ['sphere', 'torus', 'edge values'])
def test_kernels_on_the_shaped_fields(ops, name):
    f = {'sphere': lambda: mr.sphere_field()[0], 'torus': mr.torus_field, 'edge values': mr.edge_value_field}[name]()
    assert _check_against_restatement(ops, f, 0.0, name) > 100
    if name == 'sphere':                                             # a level that is no float32 is rounded to one, once
        _check_against_restatement(ops, f, 0.1, 'sphere at level 0.1')


def test_kernels_on_a_row_of_299_cubes(ops):
    """300 x 3 x 4 points: a row of 299 cubes is two chunks of 256 threads and no multiple of 64."""
    f = np.random.RandomState(7).randn(4, 3, 300).astype(np.float32)
    assert _check_against_restatement(ops, f, 0.0, '300 x 3 x 4') > 3000
    assert _check_against_restatement(ops, f, 1.5, '300 x 3 x 4, sparse') > 100


def test_kernels_on_all_256_corner_patterns(ops):
    """Every inside / outside pattern of a cube's 8 corners, as one batch along z: pattern p in the slabs 3p and 3p + 1 of a
    2 x 2 x 768-point grid, an outside slab behind each."""
    rng = np.random.RandomState(11)
    f = -rng.uniform(0.1, 1.0, (768, 2, 2)).astype(np.float32)
    for p in range(256):
        for c in range(8):
            if (p >> c) & 1:
                f[3 * p + (c >> 2), (c >> 1) & 1, c & 1] *= -1
    _check_against_restatement(ops, f, 0.0, '256 patterns')
    row_count = ops.mesh_count(T(f), 0.0).cpu().numpy()
    for p in range(256):                                             # and the count of each pattern's cube from the table
        want = 0
        for t in range(6):
            m = sum(((p >> c) & 1) << i for i, c in enumerate(mr.tet_corners(t)))
            want += int((mr.CASE_TABLE[t, m, [0, 3]] != mr.EMPTY).sum())
        assert row_count[3 * p] == want, p


def test_empty_surface(ops):
    from occnerf_amd import mesh
    f, _ = mr.sphere_field()
    fd = T(f)
    level = float(f.max()) + 1.0
    row_count, row_start, total = _device_keys(ops, fd, level)
    assert total == 0 and not bool(row_count.any())
    assert tuple(ops.mesh_emit(fd, level, row_start, 0).shape) == (0, 3)
    assert tuple(ops.mesh_vertices(torch.empty(0, device=DEV, dtype=torch.int64), fd, level, BBOX_MIN, H).shape) == (0, 3)
    verts, faces = mesh.extract_mesh(fd, level, BBOX_MIN, H)
    assert tuple(verts.shape) == (0, 3) and tuple(faces.shape) == (0, 3) and faces.dtype == torch.int32
    torch.cuda.synchronize()


def test_emit_never_writes_at_or_past_T(ops):
    f = np.random.RandomState(7).randn(4, 3, 300).astype(np.float32)
    _, want_keys = mr.extract_keys(f, 0.0)
    fd = T(f)
    _, row_start, total = _device_keys(ops, fd, 0.0)
    for short in (total - 7, total // 2, 1):
        buf = torch.full((total + 5, 3), -1, device=DEV, dtype=torch.int64)
        ops.mesh_emit(fd, 0.0, row_start, short, out=buf)
        got = buf.cpu().numpy()
        same(got[:short], want_keys[:short], f'rows below T = {short}')
        assert (got[short:] == -1).all(), short
    with pytest.raises(RuntimeError, match='mesh_vertices: keys must be int64 \\[V\\]'):
        ops.mesh_vertices(torch.zeros(2, 2, device=DEV, dtype=torch.int64), fd, 0.0, BBOX_MIN, H)
    # a key that names no edge of the grid reads nothing and gives NaN
    bad = torch.tensor([-5, 7 * f.size + 3, (f.size - 1) * 7 + 0], device=DEV, dtype=torch.int64)
    assert bool(torch.isnan(ops.mesh_vertices(bad, fd, 0.0, BBOX_MIN, H)).all())


# ------------------------------------------------------------------ the canonical field at arbitrary points
@pytest.fixture(scope='module')
def seeded():
    net, ctx = build_network(0, False, S=32)
    return net, ctx


def _query_points(ctx, n, seed):
    """Points inside the body, in the box around it, and far outside the box."""
    rng = np.random.RandomState(seed)
    base = ctx['point_base']
    third = n // 3
    q = np.concatenate([base[rng.randint(0, len(base), third)] + rng.randn(third, 3) * 0.01,
                        rng.uniform(-1.3, 1.3, (third, 3)),
                        rng.uniform(-40, 40, (n - 2 * third, 3))]).astype(np.float32)
    rng.shuffle(q)
    return q


def test_query_canonical_against_the_oracle(seeded, ops, oracle):
    """389 points (no multiple of 128): the stages query_canonical composes against the oracle's, with the bars of
    test_a_rows.py -- kNN indices equal, signed distance and hash encoding equal, aggregation 1e-6, MLP output 2e-6 (the
    random-init checkpoint's bars there) -- and then its result."""
    net, ctx = seeded
    q = _query_points(ctx, 389, 5)
    want_knn = oracle.msknn(q, ctx['point_base'], ctx['fps'], k=10)
    table = stagewise_table(ctx, oracle)
    Wg, Bg, Wc, Bc = util.canonical_mlp_params(ctx['sd'])
    want_raw, want_in = oracle.canonical_mlp(q, want_knn, ctx['point_base'], ctx['normals'], ctx['counter'], table, ctx['bound'],
                                             ctx['embeddings'], ctx['offsets'], ctx['S'], ctx['H'], Wg, Bg, Wc, Bc,
                                             want_mlp_in=True)
    c = net._context()
    enc = net.cnl_mlp.module.encoder
    pad = np.concatenate([q, np.repeat(q[-1:], (-len(q)) % 128, 0)])
    knn = ops.msknn_clustered(T(pad), len(pad) // 128, 128, c['clusters'], c['seed'])
    same(knn.cpu().numpy()[:len(q)], want_knn, 'kNN indices')
    with torch.no_grad():
        dev_table = net._point_stage(c)
    same(dev_table.cpu().numpy()[:, :35], table, 'per-point table')
    mlp_in, raw4, _ = ops.sample_features(T(pad), knn, net.point_base.detach(), c['normals'], c['unit'], net.point_counter.detach(),
                                          dev_table, c['bound32'], c['two_bound32'], enc.embeddings.detach(), enc.offsets,
                                          enc.log2_per_level_scale, enc.base_resolution)
    mi = mlp_in.cpu().numpy()[:len(q)]
    same(raw4.cpu().numpy()[:len(q), 4], want_raw[:, 4], 'signed distance')
    same(mi[:, 36:], want_in[:, 36:], 'hash encoding')
    print('\n   aggregation: max |hip - oracle|', np.abs(mi[:, :36] - want_in[:, :36]).max())
    assert np.abs(mi[:, :36] - want_in[:, :36]).max() <= 1e-6
    raw = net.query_canonical(T(q))
    assert tuple(raw.shape) == (389, 5) and raw.dtype == torch.float32 and raw.is_cuda
    got = raw.cpu().numpy()
    same(got[:, 4], want_raw[:, 4], 'query_canonical: signed distance')
    print('   raw[:, :4]: max |hip - oracle|', np.abs(got[:, :4] - want_raw[:, :4]).max())
    assert np.abs(got[:, :4] - want_raw[:, :4]).max() <= 2e-6


def test_query_canonical_is_independent_of_the_chunk(seeded):
    net, ctx = seeded
    q = T(_query_points(ctx, 9001, 6))
    one = net.query_canonical(q)
    for chunk in (4096, 128, 1000):
        assert torch.equal(net.query_canonical(q, chunk=chunk).view(torch.int32), one.view(torch.int32)), chunk
    # rows are functions of their own point: a subset, reversed
    sub = torch.arange(q.shape[0] - 1, -1, -7, device=DEV)
    assert torch.equal(net.query_canonical(q[sub].contiguous()).view(torch.int32), one[sub].view(torch.int32))
    # whatever cfg.mlp_precision says, the fp32 kernels answer
    net.cfg.mlp_precision = 'f16x3'
    try:
        assert torch.equal(net.query_canonical(q, chunk=4096).view(torch.int32), one.view(torch.int32))
    finally:
        net.cfg.mlp_precision = 'fp32'
    assert tuple(net.query_canonical(torch.empty(0, 3, device=DEV)).shape) == (0, 5)


def test_query_canonical_side_effects_and_refusals(seeded):
    net, ctx = seeded
    q = T(_query_points(ctx, 300, 7))
    net.query_canonical(q)                                           # (the per-model constants exist from here on)
    counter, version = net.point_counter.detach().clone(), net.point_counter._version
    rng_dev, rng_host = torch.cuda.get_rng_state(0), torch.get_rng_state()
    wconst, packed, orders = net._wconst, net._packed, dict(net._ray_orders)
    try:
        for mode in (True, False):
            net.train(mode)
            out = net.query_canonical(q)
            assert net.training is mode and not out.requires_grad
    finally:
        net.eval()
    assert torch.equal(net.point_counter.detach(), counter) and net.point_counter._version == version
    assert torch.equal(torch.cuda.get_rng_state(0), rng_dev) and torch.equal(torch.get_rng_state(), rng_host)
    assert net._wconst is wconst and net._packed is packed and net._ray_orders == orders
    for bad in (torch.zeros(5, 2, device=DEV), torch.zeros(15, device=DEV), torch.zeros(5, 3, device=DEV, dtype=torch.float64),
                torch.zeros(2, 5, 3, device=DEV)):
        with pytest.raises(RuntimeError, match='query_canonical: xyz must be float32 \\[N,3\\]'):
            net.query_canonical(bad)
    with pytest.raises(RuntimeError, match='query_canonical: xyz must be a CUDA'):
        net.query_canonical(torch.zeros(5, 3))


# ------------------------------------------------------------------ end to end
def test_export_mesh_end_to_end(seeded, tmp_path):
    from occnerf_amd import mesh, synth
    from occnerf_amd.image import to_8b_image
    net, ctx = seeded
    frame = synth.make_frame(img_size=8, with_rays=False)
    lo, hi = frame['cnl_bbox_min_xyz'], frame['cnl_bbox_max_xyz']
    field, h, (nx, ny, nz) = mesh.density_grid(net, lo, hi, 24)
    assert tuple(field.shape) == (nz, ny, nx) and max(nx, ny, nz) == 25 and field.dtype == torch.float32
    f = field.cpu().numpy()
    # the grid is softplus of the density logit at float32(min + i * h)
    ax = mesh.grid_axes(lo, h, (nx, ny, nz))
    pts = np.stack(np.meshgrid(ax[2], ax[1], ax[0], indexing='ij')[::-1], -1).reshape(-1, 3)
    raw = net.query_canonical(T(pts))
    assert torch.equal(torch.nn.functional.softplus(raw[:, 3]).reshape(nz, ny, nx), field)
    level = float(np.median(f))                                      # a surface exists whatever the random weights give
    infos = [mesh.export_mesh(net, str(tmp_path / name), lo, hi, resolution=24, level=level) for name in ('a', 'b')]
    info = json.loads((tmp_path / 'a' / 'mesh.json').read_text())
    assert info == infos[0] and info['level'] == float(np.float32(level)) and info['level_is_default'] is False
    assert info['grid_shape_xyz'] == [nx, ny, nz] and info['resolution'] == 24 and info['h'] == h
    assert set(info['seconds']) == {'grid', 'extract', 'colour'}
    ply = mr.parse_ply((tmp_path / 'a' / 'mesh.ply').read_bytes())
    verts, faces = np.stack([ply['x'], ply['y'], ply['z']], 1), ply['faces']
    V = verts.shape[0]
    assert V == info['vertices'] > 100 and faces.shape[0] == info['triangles'] > 100
    assert faces.min() >= 0 and faces.max() < V
    assert (verts >= lo - 1e-6).all() and (verts <= hi + 1e-6).all()
    want_verts, want_faces = mr.extract_mesh(f, level, lo.astype(np.float64), h)
    same(verts, want_verts, 'exported vertices')
    same(faces, want_faces, 'exported faces')
    with np.errstate(invalid='ignore'):
        inside = f > np.float32(level)
    on_boundary = int(inside.sum() - inside[1:-1, 1:-1, 1:-1].sum())
    assert info['inside_points_on_boundary'] == on_boundary
    assert mr.is_closed(faces) == (on_boundary == 0)
    rgb = torch.sigmoid(net.query_canonical(T(verts))[:, :3]).cpu().numpy()
    same(np.stack([ply['red'], ply['green'], ply['blue']], 1), to_8b_image(rgb), 'vertex colours')
    same(np.stack([ply['nx'], ply['ny'], ply['nz']], 1), synth.vertex_normals(verts, faces).astype(np.float32), 'normals')
    # the same inputs: the same bytes (the sidecar but for its wall times)
    assert (tmp_path / 'a' / 'mesh.ply').read_bytes() == (tmp_path / 'b' / 'mesh.ply').read_bytes()
    assert {k: v for k, v in infos[0].items() if k != 'seconds'} == {k: v for k, v in infos[1].items() if k != 'seconds'}
    # the default level and a mesh without normals
    info = mesh.export_mesh(net, str(tmp_path / 'c'), lo, hi, resolution=24, normals=False)
    assert info['level_is_default'] and info['level'] == float(np.float32(np.log(2.0) / h))
    assert 'nx' not in mr.parse_ply((tmp_path / 'c' / 'mesh.ply').read_bytes())


def test_run_py_mesh_entry_point(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, 'run.py'), '--cfg', os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml'),
           '--type', 'mesh', 'mesh.resolution', '24', 'N_samples', '16']
    out = subprocess.run(cmd, cwd=str(tmp_path), env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    folder = tmp_path / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'seeded' / 'mesh'
    info = json.loads((folder / 'mesh.json').read_text())
    ply = mr.parse_ply((folder / 'mesh.ply').read_bytes())
    assert info['resolution'] == 24 and max(info['grid_shape_xyz']) == 25 and info['level_is_default'] is True
    assert ply['x'].shape[0] == info['vertices'] and ply['faces'].shape[0] == info['triangles'] and 'nx' in ply
