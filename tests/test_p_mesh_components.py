"""GPU: the mesh clean-up.  csrc/mesh_components.hip against the numpy definition
(tests/mesh_components_restatement.py) -- labels, every record column, kept vertices and faces all EQUAL --, and
occnerf_amd.mesh.export_mesh / run.py --type mesh with mesh.components end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_components_restatement as cr
from tests import mesh_restatement as mr
from tests.gpu_util import DEV, T, build_network, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BBOX_MIN, H = np.array([-1.25, 0.5, 2.0]), 0.037
COLUMNS = ('label', 'vertices', 'triangles', 'boundary_vertices', 'smin', 'smax', 'volume6_q')
POLICIES = (('largest', False), (0.1, False), (0.1, True), ('all', True))


def _device(ops, verts, faces, lo, h, shape):
    labels, rec = ops.mesh_components(T(verts), T(faces), lo, h, shape)
    assert labels.dtype == torch.int32 and labels.is_cuda and tuple(labels.shape) == (verts.shape[0],)
    assert set(rec) == set(COLUMNS) | {'passes'}
    for k in COLUMNS:
        assert rec[k].is_cuda and rec[k].dtype == (torch.int64 if k == 'volume6_q' else torch.int32), k
    return labels, rec


def _check(ops, verts, faces, lo, h, shape, name):
    """Everything the device returns, and the filter under every policy, against the definition."""
    from occnerf_amd import mesh
    want_lab, want = cr.components(verts, faces, lo, h, shape)
    labels, rec = _device(ops, verts, faces, lo, h, shape)
    same(labels.cpu().numpy(), want_lab, f'{name}: labels')
    for k in COLUMNS:
        same(rec[k].cpu().numpy(), want[k], f'{name}: {k}')
    host = {k: rec[k].cpu().numpy() for k in COLUMNS}
    for components, drop in POLICIES:
        keep = mesh.select_components(host, components, drop)
        same(keep, cr.select(want, components, drop), f'{name}: keep flags under {components}, {drop}')
        v2, f2 = mesh.filter_mesh(T(verts), T(faces), labels, keep)
        want_v, want_f = cr.filter_mesh(verts, faces, want_lab, keep)
        assert v2.dtype == torch.float32 and f2.dtype == torch.int32 and v2.is_cuda and f2.is_cuda
        same(v2.cpu().numpy().view(np.uint32), want_v.view(np.uint32), f'{name}: kept vertices under {components}, {drop}')
        same(f2.cpu().numpy(), want_f, f'{name}: kept faces under {components}, {drop}')
    return want, rec['passes']


def _field_mesh(field, lo=BBOX_MIN, h=H):
    verts, faces = mr.extract_mesh(field, 0.0, lo, h)
    return verts, faces, tuple(field.shape[::-1])


@pytest.mark.parametrize('name', ['shell', 'shell and floater', 'torus', 'edge values', 'clipped sphere'])
def test_kernels_on_the_shaped_fields(ops, name):
    field = {'shell': cr.shell_field, 'shell and floater': cr.shell_floater_field, 'torus': mr.torus_field,
             'edge values': mr.edge_value_field, 'clipped sphere': cr.clipped_sphere_field}[name]()
    verts, faces, shape = _field_mesh(field)
    want, passes = _check(ops, verts, faces, BBOX_MIN, H, shape, name)
    assert want['label'].shape[0] == {'shell': 2, 'shell and floater': 3}.get(name, 1) and 1 <= passes <= 50
    if name == 'shell and floater':                                  # and in the units of the CPU tests, where the facts are known
        verts, faces, shape = _field_mesh(field, np.zeros(3), 1.0)
        want, _ = _check(ops, verts, faces, np.zeros(3), 1.0, shape, name + ', unit grid')
        assert want['label'].tolist()[:2] == [0, 16] and want['triangles'].tolist() == [144, 7800, 1728]


def test_kernels_on_the_random_grids(ops):
    total = 0
    for i, f in enumerate(mr.random_fields()):
        verts, faces, shape = _field_mesh(f)
        want, _ = _check(ops, verts, faces, BBOX_MIN, H, shape, f'random field {i}')
        total += want['label'].shape[0]
    assert total > 20


def test_rod_label_travels_200_cubes_in_few_passes(ops):
    verts, faces, shape = _field_mesh(cr.rod_field())
    assert faces.shape[0] == 4752
    want, passes = _check(ops, verts, faces, BBOX_MIN, H, shape, 'rod')
    print(f'\n   rod: {passes} device passes (the synchronous definition takes 9 rounds)')
    assert want['label'].tolist() == [0] and passes <= 50
    # the vertex indices shuffled and the faces permuted: other labels, the same partition, sizes and volumes
    rng = np.random.RandomState(5)
    perm = rng.permutation(verts.shape[0])                           # old index -> new index
    verts2 = np.empty_like(verts)
    verts2[perm] = verts
    faces2 = perm[faces].astype(np.int32)[rng.permutation(faces.shape[0])]
    want2, passes2 = _check(ops, verts2, faces2, BBOX_MIN, H, shape, 'rod, shuffled')
    print(f'   rod, shuffled: {passes2} device passes')
    assert passes2 <= 50
    for k in ('vertices', 'triangles', 'boundary_vertices', 'smin', 'smax', 'volume6_q'):
        same(want2[k], want[k], f'rod, shuffled against the rod: {k}')
    # two bodies under one shuffle: the partition is carried by the permutation
    verts, faces, shape = _field_mesh(cr.shell_floater_field())
    lab = cr.labels(faces, verts.shape[0])
    perm = rng.permutation(verts.shape[0])
    verts2 = np.empty_like(verts)
    verts2[perm] = verts
    faces2 = perm[faces].astype(np.int32)[rng.permutation(faces.shape[0])]
    want2, _ = _check(ops, verts2, faces2, BBOX_MIN, H, shape, 'shell and floater, shuffled')
    labels2, _ = _device(ops, verts2, faces2, BBOX_MIN, H, shape)
    got = labels2.cpu().numpy()[perm]                                # per old vertex
    for label in np.unique(lab):
        assert np.unique(got[lab == label]).size == 1
    assert np.unique(got).size == 3 and sorted(want2['triangles'].tolist()) == [144, 1728, 7800]
    assert sorted(want2['volume6_q'].tolist()) == sorted(cr.records(verts, faces, lab, BBOX_MIN, H, shape)['volume6_q'].tolist())


def test_many_roots_and_sizes_that_are_no_multiple_of_the_wave(ops):
    verts, faces = cr.disjoint_triangles(3000)
    assert verts.shape[0] % 64 and faces.shape[0] % 64 and verts.shape[0] % 256 and faces.shape[0] % 256
    want, passes = _check(ops, verts, faces, np.zeros(3), 1.0, (11, 11, 11), '3000 disjoint triangles')
    assert want['label'].shape[0] == 3007 and passes <= 3
    assert sorted(want['triangles'].tolist()) == [0] * 7 + [1] * 3000
    # hand-made: a shared vertex, a degenerate face, an unreferenced vertex; then no face at all; then nothing
    faces = np.array([[4, 1, 2], [2, 3, 0], [5, 5, 6], [10, 9, 8]], dtype=np.int32)
    verts = (np.arange(33, dtype=np.float32).reshape(11, 3) % 7 + 1)
    want, _ = _check(ops, verts, faces, np.zeros(3), 1.0, (9, 9, 9), 'hand-made')
    assert want['label'].tolist() == [0, 5, 7, 8]
    none = np.zeros((0, 3), dtype=np.int32)
    want, passes = _check(ops, verts[:4], none, np.zeros(3), 1.0, (9, 9, 9), 'no face')
    assert want['label'].tolist() == [0, 1, 2, 3] and passes == 1
    want, passes = _check(ops, verts[:0], none, np.zeros(3), 1.0, (9, 9, 9), 'nothing')
    assert want['label'].shape == (0,) and passes == 0
    # wild coordinates are held to +-2^30, NaN to the lower end
    wild = verts.copy()
    wild[1], wild[3] = [np.nan, np.inf, -np.inf], [3e9, -3e9, 1.0]
    _check(ops, wild, faces, np.zeros(3), 1.0, (9, 9, 9), 'wild coordinates')


def test_two_calls_give_the_same_bytes(ops):
    verts, faces, shape = _field_mesh(cr.shell_floater_field())
    rng = np.random.RandomState(9)
    faces = faces[rng.permutation(faces.shape[0])]
    runs = []
    for _ in range(2):
        labels, rec = _device(ops, verts, faces, BBOX_MIN, H, shape)
        runs.append([labels.cpu().numpy().tobytes()] + [rec[k].cpu().numpy().tobytes() for k in COLUMNS])
    assert runs[0] == runs[1]


def test_refusals(ops):
    verts, faces = T(np.ones((5, 3), dtype=np.float32)), T(np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32))
    with pytest.raises(RuntimeError, match='mesh_label: a face names a vertex outside \\[0, 5\\)'):
        ops.mesh_components(verts, T(np.array([[0, 1, 5]], dtype=np.int32)), np.zeros(3), 1.0, (4, 4, 4))
    with pytest.raises(RuntimeError, match='mesh_label: a face names a vertex outside'):
        ops.mesh_components(verts, T(np.array([[0, -1, 2]], dtype=np.int32)), np.zeros(3), 1.0, (4, 4, 4))
    with pytest.raises(RuntimeError, match='faces must be torch.int32'):
        ops.mesh_components(verts, faces.long(), np.zeros(3), 1.0, (4, 4, 4))
    with pytest.raises(RuntimeError, match='faces must be int32 \\[T,3\\]'):
        ops.mesh_components(verts, faces.reshape(-1), np.zeros(3), 1.0, (4, 4, 4))
    with pytest.raises(RuntimeError, match='mesh_components: verts must be a float32 \\[V,3\\]'):
        ops.mesh_components(verts.reshape(-1), faces, np.zeros(3), 1.0, (4, 4, 4))
    with pytest.raises(RuntimeError, match='must be a CUDA'):
        ops.mesh_components(verts.cpu(), faces.cpu(), np.zeros(3), 1.0, (4, 4, 4))
    with pytest.raises(RuntimeError, match='mesh_component_stats: h = 0.0 must be positive'):
        ops.mesh_components(verts, faces, np.zeros(3), 0.0, (4, 4, 4))
    # the cap on the passes is an error by name, never partial labels: a chain of 40 triangles cannot end in one pass
    chain = np.stack([np.arange(0, 80, 2), np.arange(1, 81, 2), np.arange(2, 82, 2)], 1).astype(np.int32)[::-1].copy()
    with pytest.raises(RuntimeError, match='mesh_label: no pass left the labels unchanged within max_passes = 1 '):
        ops.mesh_label(T(chain), 81, max_passes=1)
    labels, passes = ops.mesh_label(T(chain), 81)
    assert not bool(labels.any()) and 2 <= passes <= 50
    torch.cuda.synchronize()


# ------------------------------------------------------------------ end to end
QUANTILES = (0.75, 0.9, 0.95, 0.25, 0.1, 0.05, 0.6, 0.4)


@pytest.fixture(scope='module')
def seeded():
    """The seeded network, its 24-grid and two iso levels: the field's median, and the first of QUANTILES at which the
    definition finds more than one component (random weights put one sheet through the box at the median)."""
    from occnerf_amd import mesh, synth
    net, _ = build_network(0, False, S=32)
    frame = synth.make_frame(img_size=8, with_rays=False)
    lo, hi = frame['cnl_bbox_min_xyz'], frame['cnl_bbox_max_xyz']
    field, h, shape = mesh.density_grid(net, lo, hi, 24)
    f = field.cpu().numpy()
    levels = {'median': float(np.median(f))}
    for q in QUANTILES:
        level = float(np.float32(np.quantile(f, q)))
        v, fa = mr.extract_mesh(f, level, lo.astype(np.float64), h)
        found = np.unique(cr.labels(fa, v.shape[0])).size
        print(f'\n   quantile {q}: level {level:.6g}, {fa.shape[0]} triangles in {found} components')
        if found > 1:
            levels['several'] = level
            break
    assert 'several' in levels, 'no quantile of the seeded 24-grid gives more than one component'
    return net, lo, hi, f, h, shape, levels


def _ply_mesh(path):
    ply = mr.parse_ply(path.read_bytes())
    return ply, np.ascontiguousarray(np.stack([ply['x'], ply['y'], ply['z']], 1)), ply['faces']


@pytest.mark.parametrize('which', ['median', 'several'])
def test_export_mesh_keeps_the_largest_component(seeded, tmp_path, which):
    from occnerf_amd import mesh, synth
    from occnerf_amd.image import to_8b_image
    net, lo, hi, f, h, shape, levels = seeded
    level = levels[which]
    kw = dict(resolution=24, level=level)
    kept = {}
    infos = [mesh.export_mesh(net, str(tmp_path / name), lo, hi, components='largest', keep=(kept if name == 'a' else None), **kw)
             for name in ('a', 'b')]
    info = json.loads((tmp_path / 'a' / 'mesh.json').read_text())
    assert info == infos[0] and set(info['seconds']) == {'grid', 'extract', 'colour', 'components'}
    ply, verts, faces = _ply_mesh(tmp_path / 'a' / 'mesh.ply')
    assert info['vertices'] == verts.shape[0] > 100 and info['triangles'] == faces.shape[0] > 100
    assert np.unique(cr.labels(faces, verts.shape[0])).tolist() == [0]          # exactly one component in what was written
    lo64 = lo.astype(np.float64)
    all_v, all_f = mr.extract_mesh(f, level, lo64, h)
    lab, rec = cr.components(all_v, all_f, lo64, h, shape)
    assert (rec['label'].shape[0] > 1) == (which == 'several')
    want_v, want_f = cr.filter_mesh(all_v, all_f, lab, cr.select(rec, 'largest'))
    same(verts.view(np.uint32), want_v.view(np.uint32), 'exported vertices')
    same(faces, want_f, 'exported faces')
    c = info['components']
    assert info['extracted_vertices'] == all_v.shape[0] and info['extracted_triangles'] == all_f.shape[0]
    assert c['policy'] == {'components': 'largest', 'drop_cavities': False} and c['found'] == rec['label'].shape[0]
    assert c['kept'] == 1 and c['dropped_vertices'] == all_v.shape[0] - verts.shape[0]
    assert c['dropped_triangles'] == all_f.shape[0] - faces.shape[0] and c['cavities_dropped'] == 0 and 1 <= c['passes'] <= 50
    assert (c['dropped_triangles'] > 0) == (which == 'several')
    assert len(c['largest']) == min(16, c['found']) and c['largest'][0]['verdict'] == 'kept'
    assert c['largest'][0]['triangles'] == faces.shape[0] == int(rec['triangles'].max())
    assert all(r['verdict'] == 'small' for r in c['largest'][1:])
    rgb = torch.sigmoid(net.query_canonical(T(verts))[:, :3]).cpu().numpy()
    same(np.stack([ply['red'], ply['green'], ply['blue']], 1), to_8b_image(rgb), 'vertex colours')
    same(np.stack([ply['nx'], ply['ny'], ply['nz']], 1), synth.vertex_normals(verts, faces).astype(np.float32), 'normals')
    same(kept['verts'].cpu().numpy().view(np.uint32), verts.view(np.uint32), 'keep: vertices')
    same(kept['faces'], faces, 'keep: faces')
    assert (tmp_path / 'a' / 'mesh.ply').read_bytes() == (tmp_path / 'b' / 'mesh.ply').read_bytes()
    assert {k: v for k, v in infos[0].items() if k != 'seconds'} == {k: v for k, v in infos[1].items() if k != 'seconds'}
    # the defaults spelt out: the bytes and the sidecar keys of an export without the keywords
    plain = mesh.export_mesh(net, str(tmp_path / 'c'), lo, hi, **kw)
    spelt = mesh.export_mesh(net, str(tmp_path / 'd'), lo, hi, components='all', drop_cavities=False, **kw)
    assert (tmp_path / 'c' / 'mesh.ply').read_bytes() == (tmp_path / 'd' / 'mesh.ply').read_bytes()
    assert set(plain) == set(spelt) and 'components' not in spelt and 'extracted_vertices' not in spelt
    assert set(spelt['seconds']) == {'grid', 'extract', 'colour'} and plain['vertices'] == all_v.shape[0]
    # cavities alone, and a policy that drops everything but what it must keep, on a level without a surface
    cav = mesh.export_mesh(net, str(tmp_path / 'e'), lo, hi, drop_cavities=True, **kw)
    want_keep = cr.select(rec, 'all', True)
    assert cav['components']['kept'] == int(want_keep.sum()) and cav['triangles'] == int(rec['triangles'][want_keep].sum())
    empty = mesh.export_mesh(net, str(tmp_path / 'f'), lo, hi, resolution=24, level=float(f.max()) + 1.0, components='largest')
    assert empty['vertices'] == 0 and empty['triangles'] == 0 and empty['components']['found'] == 0
    assert mr.parse_ply((tmp_path / 'f' / 'mesh.ply').read_bytes())['faces'].shape == (0, 3)


def test_posing_gets_the_clean_mesh(seeded, tmp_path):
    """A plausibility check without a threshold on the size of the drop: the posed file has the kept vertex count and the
    flagged counts of posed.json do not rise when the detached blobs are gone."""
    from occnerf_amd import mesh
    net, lo, hi, f, h, shape, levels = seeded
    level = levels['several']
    source = mesh.PoseFrames(None, total_frames=8)
    flagged = {}
    for name, components in (('all', 'all'), ('largest', 'largest')):
        kept = {}
        info = mesh.export_mesh(net, str(tmp_path / name), lo, hi, resolution=24, level=level, keep=kept, components=components)
        posed = mesh.export_posed(net, str(tmp_path / name), kept, source, [3], non_rigid=False)
        ply = mr.parse_ply((tmp_path / name / 'posed' / 'frame_000003.ply').read_bytes())
        assert posed['vertices'] == info['vertices'] == ply['x'].shape[0] and ply['faces'].shape[0] == info['triangles']
        fr = posed['frames'][0]
        flagged[name] = (fr['not_converged'], fr['no_bone'], info['vertices'])
    print(f'\n   (not converged, no bone, vertices): all {flagged["all"]}, largest {flagged["largest"]}')
    assert flagged['largest'][2] < flagged['all'][2]
    assert flagged['largest'][0] <= flagged['all'][0] and flagged['largest'][1] <= flagged['all'][1]


def test_run_py_mesh_components_largest(seeded, tmp_path):
    level = seeded[6]['several']
    cmd = [sys.executable, os.path.join(ROOT, 'run.py'), '--cfg', os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml'),
           '--type', 'mesh', 'mesh.resolution', '24', 'mesh.components', 'largest', 'mesh.level', repr(level), 'N_samples', '16']
    out = subprocess.run(cmd, cwd=str(tmp_path), env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    folder = tmp_path / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'seeded' / 'mesh'
    info = json.loads((folder / 'mesh.json').read_text())
    _, verts, faces = _ply_mesh(folder / 'mesh.ply')
    assert info['components']['kept'] == 1 and info['components']['policy']['components'] == 'largest'
    assert info['components']['found'] > 1 and info['components']['dropped_triangles'] > 0
    assert info['vertices'] == verts.shape[0] > 100 and info['triangles'] == faces.shape[0]
    assert info['extracted_vertices'] >= info['vertices']
    assert np.unique(cr.labels(faces, verts.shape[0])).tolist() == [0]
    assert 'components kept' in out.stdout
