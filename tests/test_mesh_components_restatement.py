"""CPU: the numpy definition of the mesh clean-up (tests/mesh_components_restatement.py) against facts
that do not come from it -- the fields' geometry, mesh_restatement's closedness test and float64 signed volume -- and the
host side of occnerf_amd.mesh: select_components against the definition's selection, the refusals by name, the C entries'
argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import mesh_components_restatement as cr
from tests import mesh_restatement as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, H = np.zeros(3), 1.0


def _mesh(field):
    verts, faces = mr.extract_mesh(field, 0.0, LO, H)
    return verts, faces, tuple(field.shape[::-1])


@pytest.fixture(scope='module')
def shell():
    verts, faces, shape = _mesh(cr.shell_field())
    lab, rec = cr.components(verts, faces, LO, H, shape)
    return verts, faces, lab, rec


@pytest.fixture(scope='module')
def floater():
    verts, faces, shape = _mesh(cr.shell_floater_field())
    lab, rec = cr.components(verts, faces, LO, H, shape)
    return verts, faces, lab, rec


def _component_faces(faces, lab, label):
    return faces[lab[faces[:, 0]] == label]


def _check_volumes(verts, faces, lab, rec):
    """volume6_q against the float64 signed volume of every component, to the bound the snapping alone gives."""
    vol = cr.volume(rec)
    for r, label in enumerate(rec['label']):
        sub = _component_faces(faces, lab, label)
        want, bound = mr.signed_volume(verts, sub), cr.volume_snap_bound(verts, sub, LO, H)
        assert abs(vol[r] - want) <= bound, (label, vol[r], want, bound)
        assert bound < 1e-3 * max(abs(want), 1.0) + 0.05                  # (the bound itself is tight enough to mean something)


def test_shell_has_an_outer_surface_and_a_cavity(shell):
    verts, faces, lab, rec = shell
    assert rec['label'].tolist() == [0, int(rec['label'][1])] and rec['triangles'].tolist() == [7800, 1728]
    assert int(rec['vertices'].sum()) == verts.shape[0] and rec['boundary_vertices'].tolist() == [0, 0]
    vol = cr.volume(rec)
    assert abs(vol[0] - 2377.8) < 0.05 and abs(vol[1] + 280.1) < 0.05
    _check_volumes(verts, faces, lab, rec)
    # the geometry: matter for 4.1 < r < 8.3 around (10, 10, 10), so the boxes are those radii about the centre
    for r, radius in ((0, 8.3), (1, 4.1)):
        assert np.abs(rec['smin'][r] / 1024 - (10 - radius)).max() < 0.25 and np.abs(rec['smax'][r] / 1024 - (10 + radius)).max() < 0.25
    assert cr.is_cavity(rec).tolist() == [False, True]
    for label in rec['label']:
        assert mr.is_closed(_component_faces(faces, lab, label))
    keep = cr.select(rec, 'all', drop_cavities=True)
    assert keep.tolist() == [True, False]
    v2, f2 = cr.filter_mesh(verts, faces, lab, keep)
    assert v2.shape[0] == rec['vertices'][0] and f2.shape[0] == 7800 and mr.is_closed(f2)
    assert f2.min() == 0 and f2.max() == v2.shape[0] - 1
    assert np.array_equal(v2[f2], verts[_component_faces(faces, lab, 0)])       # the same triangles in the same order
    assert cr.labels(f2, v2.shape[0]).max() == 0


def test_largest_is_not_label_zero(floater):
    verts, faces, lab, rec = floater
    assert rec['label'].tolist()[:2] == [0, 16] and rec['triangles'].tolist() == [144, 7800, 1728]
    vol = cr.volume(rec)
    assert abs(vol[0] - 13.6) < 0.05 and abs(vol[1] - 2377.8) < 0.05 and abs(vol[2] + 280.1) < 0.05
    _check_volumes(verts, faces, lab, rec)
    assert cr.select(rec, 'largest').tolist() == [False, True, False]
    assert cr.select(rec, 0.1).tolist() == [False, True, True]
    assert cr.select(rec, 0.1, drop_cavities=True).tolist() == [False, True, False]
    assert cr.select(rec, 'all').tolist() == [True, True, True]
    assert cr.select(rec, 1.0).tolist() == [False, True, False]
    v2, f2 = cr.filter_mesh(verts, faces, lab, cr.select(rec, 'largest'))
    assert f2.shape[0] == 7800 and mr.is_closed(f2) and np.array_equal(v2, verts[lab == 16])


def test_random_fields_sum_to_the_whole_mesh():
    seen = set()
    for f in mr.random_fields():
        verts, faces, shape = _mesh(f)
        lab, rec = cr.components(verts, faces, LO, H, shape)
        C = rec['label'].shape[0]
        seen.add(C)
        assert 1 <= C <= 3 and (np.diff(rec['label']) > 0).all()
        assert int(rec['triangles'].sum()) == faces.shape[0] and int(rec['vertices'].sum()) == verts.shape[0]
        assert (rec['boundary_vertices'] == 0).all()
        for label in rec['label']:
            assert mr.is_closed(_component_faces(faces, lab, label))
            assert label == np.nonzero(lab == label)[0].min()
        _check_volumes(verts, faces, lab, rec)
        whole, bound = mr.signed_volume(verts, faces), cr.volume_snap_bound(verts, faces, LO, H)
        assert abs(cr.volume(rec).sum() - whole) <= bound
        # the labels are the components of the vertex graph: no face joins two of them
        assert (lab[faces[:, 0]] == lab[faces[:, 1]]).all() and (lab[faces[:, 0]] == lab[faces[:, 2]]).all()
    assert len(seen) > 1


def test_hand_made_faces():
    # two triangles sharing one vertex; a degenerate face joining 5 and 6; vertex 7 unreferenced; 8, 9, 10 a third triangle
    faces = np.array([[4, 1, 2], [2, 3, 0], [5, 5, 6], [10, 9, 8]], dtype=np.int32)
    verts = np.arange(33, dtype=np.float32).reshape(11, 3) % 7 + 1
    lab = cr.labels(faces, 11)
    assert lab.tolist() == [0, 0, 0, 0, 0, 5, 5, 7, 8, 8, 8] and lab.dtype == np.int32
    rec = cr.records(verts, faces, lab, LO, H, (9, 9, 9))
    assert rec['label'].tolist() == [0, 5, 7, 8]
    assert rec['vertices'].tolist() == [5, 2, 1, 3] and rec['triangles'].tolist() == [2, 1, 0, 1]
    assert rec['volume6_q'][1] == 0 and rec['volume6_q'][2] == 0
    s = cr.snapped(verts, LO, H)
    assert np.array_equal(s, (verts.astype(np.int64) * 1024))
    assert np.array_equal(rec['smin'][2], s[7]) and np.array_equal(rec['smax'][2], s[7])
    want = int(round(np.linalg.det(s[[10, 9, 8]].astype(np.float64))))
    assert rec['volume6_q'][3] == want
    # ties in size go to the smaller label: components 5 and 8 both have one triangle once component 0 is gone
    v2, f2 = cr.filter_mesh(verts, faces, lab, [False, True, True, True])
    lab2 = cr.labels(f2, v2.shape[0])
    rec2 = cr.records(v2, f2, lab2, LO, H, (9, 9, 9))
    assert rec2['triangles'].tolist() == [1, 0, 1] and cr.select(rec2, 'largest').tolist() == [True, False, False]
    assert f2.tolist() == [[0, 0, 1], [5, 4, 3]] and np.array_equal(v2, verts[5:])
    # no triangle at all: every vertex its own component; no vertex: nothing
    lab = cr.labels(np.zeros((0, 3), np.int32), 4)
    rec = cr.records(verts[:4], np.zeros((0, 3), np.int32), lab, LO, H, (9, 9, 9))
    assert lab.tolist() == [0, 1, 2, 3] and rec['triangles'].tolist() == [0] * 4 and rec['vertices'].tolist() == [1] * 4
    assert cr.select(rec, 'largest').tolist() == [True, False, False, False] and cr.select(rec, 0.5).all()
    v2, f2 = cr.filter_mesh(verts[:4], np.zeros((0, 3), np.int32), lab, [False] * 4)
    assert v2.shape == (0, 3) and f2.shape == (0, 3)
    rec = cr.records(verts[:0], np.zeros((0, 3), np.int32), cr.labels(np.zeros((0, 3), np.int32), 0), LO, H, (9, 9, 9))
    assert rec['label'].shape == (0,) and cr.select(rec, 'largest').shape == (0,)


def test_snapping_rounds_to_even_and_holds_wild_values():
    verts = np.array([[0.5 / 1024, 1.5 / 1024, 2.5 / 1024], [np.nan, np.inf, -np.inf], [3e9, -3e9, 1.0]], dtype=np.float32)
    s = cr.snapped(verts, LO, H)
    assert s[0].tolist() == [0, 2, 2]
    assert s[1].tolist() == [-(1 << 30), 1 << 30, -(1 << 30)] and s[2].tolist() == [1 << 30, -(1 << 30), 1024]
    # lo and h enter in float64, one rounding per operator
    v = np.array([[0.1, 0.2, 0.3]], dtype=np.float32)
    lo, h = np.array([-1.25, 0.5, 2.0]), 0.037
    want = [int(np.rint(((np.float64(v[0, a]) - lo[a]) / h) * 1024.0)) for a in range(3)]
    assert cr.snapped(v, lo, h)[0].tolist() == want


def test_a_component_that_touches_the_boundary_is_never_a_cavity():
    verts, faces, shape = _mesh(cr.clipped_sphere_field())
    lab, rec = cr.components(verts, faces, LO, H, shape)
    assert rec['label'].tolist() == [0] and rec['boundary_vertices'][0] > 0 and not mr.is_closed(faces)
    assert rec['smin'][0, 0] == 0
    assert rec['boundary_vertices'][0] == int((verts[:, 0] == 0).sum())
    assert cr.select(rec, 'all', drop_cavities=True).tolist() == [True]
    flipped = faces[:, ::-1].copy()                                       # the other winding: the sign turns, the verdict stays
    rec2 = cr.records(verts, flipped, lab, LO, H, shape)
    assert rec2['volume6_q'][0] == -rec['volume6_q'][0] and rec2['volume6_q'][0] < 0
    assert not cr.is_cavity(rec2).any() and cr.select(rec2, 'all', drop_cavities=True).tolist() == [True]
    # the same sphere moved off the boundary and wound inside out is one
    verts, faces, shape = _mesh(mr.sphere_field()[0])
    lab, rec = cr.components(verts, faces[:, ::-1], LO, H, shape)
    assert cr.is_cavity(rec).tolist() == [True] and cr.select(rec, 'largest', drop_cavities=True).tolist() == [False]


def test_rod_takes_nine_synchronous_rounds():
    verts, faces, shape = _mesh(cr.rod_field())
    rounds = []
    lab = cr.labels(faces, verts.shape[0], rounds)
    assert faces.shape[0] == 4752 and mr.is_closed(faces) and (lab == 0).all() and rounds == [9]


# ------------------------------------------------------------------ the package's host side
def test_select_components_equals_the_definition(shell, floater):
    from occnerf_amd import mesh
    for _, _, _, rec in (shell, floater):
        for components in ('all', 'largest', 0.1, 0.5, 1, 1.0, 0.0185, np.float32(0.25)):
            for drop in (False, True):
                got = mesh.select_components(rec, components, drop)
                assert got.dtype == bool and np.array_equal(got, cr.select(rec, components, drop)), (components, drop)
    rec = floater[3]
    assert mesh.component_verdicts(rec, 0.1, True) == ['small', 'kept', 'cavity']
    assert mesh.component_verdicts(rec, 'largest', True) == ['small', 'kept', 'small']
    ties = {'triangles': np.array([3, 7, 7, 0]), 'boundary_vertices': np.zeros(4, np.int32), 'volume6_q': np.ones(4, np.int64)}
    assert mesh.select_components(ties, 'largest').tolist() == [False, True, False, False]
    assert mesh.select_components(ties, 1.0).tolist() == [False, True, True, False]
    empty = {'triangles': np.zeros(0, np.int32), 'boundary_vertices': np.zeros(0, np.int32), 'volume6_q': np.zeros(0, np.int64)}
    assert mesh.select_components(empty, 'largest', True).shape == (0,)
    report = mesh.components_report({**rec, 'label': rec['label']}, mesh.component_verdicts(rec, 0.1, True), 0.1, True, 5, 0.5,
                                    [1.0, 2.0, 3.0])
    assert report['found'] == 3 and report['kept'] == 1 and report['cavities_dropped'] == 1 and report['passes'] == 5
    assert report['dropped_triangles'] == 144 + 1728 and report['dropped_vertices'] == int(rec['vertices'][[0, 2]].sum())
    assert [r['triangles'] for r in report['largest']] == [7800, 1728, 144]
    assert [r['verdict'] for r in report['largest']] == ['kept', 'cavity', 'small']
    assert abs(report['largest'][0]['volume_m3'] - 2377.81 * 0.125) < 0.01
    assert np.allclose(report['largest'][0]['box_min'], np.array([1.0, 2.0, 3.0]) + rec['smin'][1] / 1024 * 0.5)


@pytest.mark.parametrize('bad', ['biggest', '', 0, 0.0, -0.5, 1.5, float('nan'), True, None, [0.5]])
def test_bad_components_are_refused_by_name(bad, shell):
    from occnerf_amd import mesh
    with pytest.raises(RuntimeError, match=r'mesh\.components'):
        mesh.select_components(shell[3], bad, False)
    with pytest.raises(RuntimeError, match=r'mesh\.components'):                   # before anything is touched: no network here
        mesh.export_mesh(None, '/nonexistent', [0, 0, 0], [1, 1, 1], components=bad)


def test_bad_drop_cavities_is_refused_by_name(shell):
    from occnerf_amd import mesh
    for bad in ('yes', 1, None):
        with pytest.raises(RuntimeError, match=r'mesh\.drop_cavities'):
            mesh.select_components(shell[3], 'all', bad)
        with pytest.raises(RuntimeError, match=r'mesh\.drop_cavities'):
            mesh.export_mesh(None, '/nonexistent', [0, 0, 0], [1, 1, 1], drop_cavities=bad)


def test_config_defaults_and_wiring():
    from occnerf_amd import _lib
    from occnerf_amd.config import default_cfg
    m = default_cfg().mesh
    assert m.components == 'all' and m.drop_cavities is False
    cfg = default_cfg()
    cfg.merge_from_list(['mesh.components', 'largest', 'mesh.drop_cavities', 'True'])
    assert cfg.mesh.components == 'largest' and cfg.mesh.drop_cavities is True
    cfg.merge_from_list(['mesh.components', '0.25'])
    assert cfg.mesh.components == 0.25
    assert _lib.ABI_VERSION == 5
    for name in ('occnerf_mesh_label_pass', 'occnerf_mesh_component_stats'):
        assert name in _lib.SIGNATURES
    make = open(os.path.join(ROOT, 'occnerf_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\bmesh_components\.hip\b', make, flags=re.M)


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    from occnerf_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def refused(rc, name, word):
        msg = lib.occnerf_last_error()
        assert rc != 0 and msg.startswith(name.encode()) and word.encode() in msg, (rc, msg)
    refused(lib.occnerf_mesh_label_pass(p, 4, 8, p, None, None), 'mesh_label_pass', 'null')
    refused(lib.occnerf_mesh_label_pass(p, 4, 8, None, p, None), 'mesh_label_pass', 'null')
    refused(lib.occnerf_mesh_label_pass(None, 4, 8, p, p, None), 'mesh_label_pass', 'null')
    refused(lib.occnerf_mesh_label_pass(p, -1, 8, p, p, None), 'mesh_label_pass', '2^31')
    refused(lib.occnerf_mesh_label_pass(p, 4, 1 << 31, p, p, None), 'mesh_label_pass', '2^31')
    assert lib.occnerf_mesh_label_pass(None, 0, 0, None, p, None) == 0
    stats = lib.occnerf_mesh_component_stats
    refused(stats(p, 8, p, 4, p, 2, None, 1.0, 4, 4, 4, p, p, p, None), 'mesh_component_stats', 'null')
    refused(stats(None, 8, p, 4, p, 2, p, 1.0, 4, 4, 4, p, p, p, None), 'mesh_component_stats', 'null')
    refused(stats(p, 8, p, 4, p, 2, p, 1.0, 4, 4, 4, p, p, None, None), 'mesh_component_stats', 'null')
    refused(stats(p, 8, p, 4, p, 9, p, 1.0, 4, 4, 4, p, p, p, None), 'mesh_component_stats', 'C=9')
    refused(stats(p, 8, p, 4, p, 2, p, 0.0, 4, 4, 4, p, p, p, None), 'mesh_component_stats', 'h=0')
    refused(stats(p, 8, p, 4, p, 2, p, float('nan'), 4, 4, 4, p, p, p, None), 'mesh_component_stats', 'h=')
    refused(stats(p, 8, p, 4, p, 2, p, 1.0, 4, 1, 4, p, p, p, None), 'mesh_component_stats', 'bad grid')
    refused(stats(p, 8, p, 4, p, 2, p, 1.0, 4, 4, (1 << 20) + 1, p, p, p, None), 'mesh_component_stats', 'bad grid')
    assert stats(None, 0, None, 0, None, 0, p, 1.0, 4, 4, 4, None, None, None, None) == 0
