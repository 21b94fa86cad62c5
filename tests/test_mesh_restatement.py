"""CPU: the numpy definition of the mesh extraction (tests/mesh_restatement.py) has the properties the
definition promises -- orientation, closedness, topology, the treatment of ties and NaN -- and what surrounds the kernels works
without a GPU: the case table compiled into csrc/mesh.hip is the restatement's, the PLY writer round-trips, the default level,
the grid rule, and the refusals of the C entries and the wrappers."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import mesh_restatement as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_single_tetrahedron_all_sign_patterns():
    """Each of the 6 tetrahedra x 16 sign patterns: 0 / 1 / 2 triangles, every vertex on an edge between an inside and an
    outside corner, normals from the inside corners to the outside ones -- with crossings anywhere on the edges, not only
    at the midpoints the table was oriented with."""
    rng = np.random.RandomState(0)
    for t in range(6):
        cs = mr.tet_corners(t)
        assert cs[0] == 0 and cs[3] == 7 and len(set(cs)) == 4
        for m in range(16):
            n_in = bin(m).count('1')
            codes = mr.CASE_TABLE[t, m]
            n_tri = int((codes[[0, 3]] != mr.EMPTY).sum())
            assert n_tri == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[n_in]
            if n_tri == 0:
                continue
            for _ in range(8):
                f = np.full((2, 2, 2), np.nan, dtype=np.float32)
                mag = rng.uniform(0.05, 1.0, 4)
                for i, c in enumerate(cs):
                    f[(c >> 2) & 1, (c >> 1) & 1, c & 1] = mag[i] if (m >> i) & 1 else -mag[i]
                pos = {c: np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], float) for c in cs}
                inside = [pos[c] for i, c in enumerate(cs) if (m >> i) & 1]
                outside = [pos[c] for i, c in enumerate(cs) if not (m >> i) & 1]
                want = np.mean(outside, 0) - np.mean(inside, 0)
                for k in range(n_tri):
                    keys = []
                    for code in codes[3 * k:3 * k + 3]:
                        c, kind = int(code) >> 3, int(code) & 7
                        assert c in cs and (c + kind + 1) in cs                 # an edge of this tetrahedron
                        assert ((m >> cs.index(c)) & 1) != ((m >> cs.index(c + kind + 1)) & 1)      # that crosses the level
                        keys.append(((c >> 2) * 4 + ((c >> 1) & 1) * 2 + (c & 1)) * 7 + kind)
                    q = mr.vertices(np.array(keys), f, 0.0, [0, 0, 0], 1.0).astype(np.float64)
                    assert np.dot(np.cross(q[1] - q[0], q[2] - q[0]), want) > 0, (t, m, k)


def test_case_table_in_the_kernel_source_is_the_restatement():
    src = open(os.path.join(ROOT, 'occnerf_amd', 'csrc', 'mesh.hip')).read()
    body = re.search(r'kCaseTable\[kMeshTableBytes\] = \{(.*?)\};', src, flags=re.S).group(1)
    body = re.sub(r'//[^\n]*', '', body)
    got = np.array([int(x, 16) for x in re.findall(r'0x[0-9A-Fa-f]{2}', body)], dtype=np.uint8)
    assert got.size == 6 * 16 * 6 and np.array_equal(got.reshape(6, 16, 6), mr.CASE_TABLE)
    mids = re.search(r'kTetMid\[kMeshTets\]\[2\] = \{(.*?)\};', src, flags=re.S).group(1)
    assert [int(x) for x in re.findall(r'\d+', mids)] == [c for t in range(6) for c in mr.tet_corners(t)[1:3]]


def test_closedness_of_random_fields():
    fields = mr.random_fields()
    assert len(fields) == 20 and fields[0].shape == (7, 6, 5)
    total = 0
    for f in fields:
        row_count, tri_keys = mr.extract_keys(f, 0.0)
        assert int(row_count.sum()) == tri_keys.shape[0] and row_count.shape == (6 * 5,)
        _, faces = mr.weld(tri_keys)
        assert faces.shape[0] > 0 and mr.is_closed(faces)
        total += faces.shape[0]
    assert total > 1000


def test_triangle_order_is_z_y_x_tetrahedron():
    """The first key of a triangle names an edge of its cube: the cubes ascend in (z, y, x) through the list, and the row
    counts are those of the (z, y) rows."""
    f = mr.random_fields()[3]
    nz, ny, nx = f.shape
    row_count, tri_keys = mr.extract_keys(f, 0.0)
    lo = tri_keys // 7
    z, y, x = lo // (nx * ny), lo // nx % ny, lo % nx
    cube = (z.min(1) * (ny - 1) + y.min(1)) * (nx - 1) + x.min(1)          # every triangle touches its cube's lo corner planes
    assert (np.diff(cube) >= 0).all()
    assert np.array_equal(np.bincount(cube // (nx - 1), minlength=row_count.size), row_count)
    assert np.bincount(cube).max() <= 12


def test_sphere_and_torus_topology():
    f, c = mr.sphere_field()
    assert f.shape == (17, 17, 17)
    verts, faces = mr.extract_mesh(f, 0.0, [0, 0, 0], 1.0)
    assert mr.is_closed(faces)
    assert mr.euler_characteristic(verts.shape[0], faces) == 2
    vol = mr.signed_volume(verts, faces)
    assert 0.9 * (4 / 3 * math.pi * 5.3 ** 3) < vol < 4 / 3 * math.pi * 5.3 ** 3          # inscribed: below the ball's volume
    tri = verts[faces].astype(np.float64)
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.einsum('ij,ij->i', normal, tri.mean(1) - c) > 0).all()
    # the box offset and the voxel size move the vertices, not the faces
    v2, f2 = mr.extract_mesh(f, 0.0, [-1.5, 0.25, 3.0], 0.125)
    assert np.array_equal(f2, faces) and np.abs(v2 - (verts * 0.125 + np.array([-1.5, 0.25, 3.0]))).max() < 1e-5
    tv, tf = mr.extract_mesh(mr.torus_field(), 0.0, [0, 0, 0], 1.0)
    assert mr.is_closed(tf) and mr.euler_characteristic(tv.shape[0], tf) == 0


def test_exact_level_and_nan_corners_are_outside():
    f = mr.edge_value_field()
    assert f[4, 4, 6] == 0.0 and np.isnan(f[4, 6, 4])
    verts, faces = mr.extract_mesh(f, 0.0, [0, 0, 0], 1.0)
    assert mr.is_closed(faces) and np.isfinite(verts).all()
    for p in ((4, 4, 6), (4, 6, 4)):                                  # the same faces as with a plainly outside value there
        g = f.copy()
        g[p] = -1e-3
        assert np.array_equal(mr.extract_mesh(g, 0.0, [0, 0, 0], 1.0)[1], faces)
        g[p] = 1e-3                                                   # ... and other faces with an inside one
        assert not np.array_equal(mr.extract_mesh(g, 0.0, [0, 0, 0], 1.0)[1].shape, faces.shape) or \
            not np.array_equal(mr.extract_mesh(g, 0.0, [0, 0, 0], 1.0)[1], faces)
    # the vertices around the exact-level corner sit on it (t = 1 from an inside lo end, t = 0 from the corner as lo end)
    near = np.abs(verts.astype(np.float64) - np.array([6.0, 4.0, 4.0])).max(1) == 0
    assert near.sum() >= 1
    # the NaN corner's edges put their vertex at the midpoint
    vkeys, _ = mr.weld(mr.extract_keys(f, 0.0)[1])
    nan_lin = (4 * 9 + 6) * 9 + 4
    lo, kind = vkeys // 7, vkeys % 7 + 1
    other = lo + (kind & 1) + ((kind >> 1) & 1) * 9 + (kind >> 2) * 81
    on_nan = (lo == nan_lin) | (other == nan_lin)
    assert on_nan.sum() >= 1
    a = np.stack([lo % 9, lo // 9 % 9, lo // 81], 1)[on_nan].astype(np.float64)
    d = np.stack([kind & 1, (kind >> 1) & 1, kind >> 2], 1)[on_nan].astype(np.float64)
    assert np.array_equal(verts[on_nan], (a + 0.5 * d).astype(np.float32))


def test_empty_and_degenerate_inputs():
    f, _ = mr.sphere_field()
    row_count, tri_keys = mr.extract_keys(f, float(f.max()) + 1.0)
    assert tri_keys.shape == (0, 3) and not row_count.any()
    verts, faces = mr.extract_mesh(f, float(f.max()), [0, 0, 0], 1.0)            # the level equal to the maximum: strict
    assert verts.shape == (0, 3) and faces.shape == (0, 3)
    verts, faces = mr.extract_mesh(np.full((2, 2, 2), np.nan, np.float32), 0.0, [0, 0, 0], 1.0)
    assert verts.shape == (0, 3) and faces.shape == (0, 3)
    verts, faces = mr.extract_mesh(np.ones((2, 3, 4), np.float32), 0.0, [0, 0, 0], 1.0)          # everything inside
    assert verts.shape == (0, 3) and faces.shape == (0, 3)


def test_ply_round_trip_and_byte_identity(tmp_path):
    from occnerf_amd import mesh
    from occnerf_amd.synth import vertex_normals
    f, _ = mr.sphere_field()
    verts, faces = mr.extract_mesh(f, 0.0, [-1.0, -2.0, -3.0], 0.25)
    colors = (np.random.RandomState(1).rand(verts.shape[0], 3) * 255).astype(np.uint8)
    normals = vertex_normals(verts, faces).astype(np.float32)
    for name, nrm in (('a.ply', normals), ('b.ply', normals), ('c.ply', None)):
        mesh.write_ply(str(tmp_path / name), verts, faces, colors, nrm)
    a, b, c = ((tmp_path / n).read_bytes() for n in ('a.ply', 'b.ply', 'c.ply'))
    assert a == b
    pa, pc = mr.parse_ply(a), mr.parse_ply(c)
    for p in (pa, pc):
        assert np.array_equal(np.stack([p['x'], p['y'], p['z']], 1), verts)
        assert np.array_equal(np.stack([p['red'], p['green'], p['blue']], 1), colors)
        assert np.array_equal(p['faces'], faces) and p['faces'].dtype == np.dtype('<i4')
    assert np.array_equal(np.stack([pa['nx'], pa['ny'], pa['nz']], 1), normals) and 'nx' not in pc
    assert len(a) - len(c) == 12 * verts.shape[0] + len(b'property float nx\n') * 3


def test_default_level_grid_rule_and_config():
    from occnerf_amd import mesh
    from occnerf_amd.config import default_cfg
    from occnerf_amd.synth import make_frame
    m = default_cfg().mesh
    assert (m.resolution, m.level, m.normals, m.chunk) == (256, None, True, 2097152)
    frame = make_frame(img_size=8, with_rays=False)
    lo, hi = frame['cnl_bbox_min_xyz'], frame['cnl_bbox_max_xyz']
    for res in (256, 24, 7, 100, 255):
        h, n = mesh.grid_shape(lo, hi, res)
        ext = hi.astype(np.float64) - lo.astype(np.float64)
        assert h == ext.max() / res and mesh.default_level(h) == math.log(2.0) / h
        assert max(n) == res + 1 and n[int(np.argmax(ext))] == res + 1          # the longest axis is never rounded down
        axes = mesh.grid_axes(lo, h, n)
        for a in range(3):
            assert axes[a].dtype == np.float32 and axes[a][0] == lo[a] and len(axes[a]) == n[a]
            assert axes[a][-1] <= hi[a] + 1e-6 and axes[a][-1] > hi[a] - h - 1e-6
        assert n[0] * n[1] * n[2] < 1 << 31
    assert math.isclose(1.0 - math.exp(-mesh.default_level(0.01) * 0.01), 0.5, rel_tol=1e-15)
    h, n = mesh.grid_shape([0, 0, 0], [1, 1, 1], 3)
    assert n == (4, 4, 4)                                                         # equal extents: every axis by the rule
    with pytest.raises(RuntimeError, match='2\\^31'):
        mesh.grid_shape([0, 0, 0], [1, 1, 1], 1300)
    with pytest.raises(RuntimeError, match='positive'):
        mesh.grid_shape([0, 0, 0], [1, 0, 1], 8)


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
    refused(lib.occnerf_mesh_count(None, 4, 4, 4, 0.0, p, None), 'mesh_count', 'null')
    refused(lib.occnerf_mesh_count(p, 4, 4, 4, 0.0, None, None), 'mesh_count', 'null')
    refused(lib.occnerf_mesh_emit(None, 4, 4, 4, 0.0, p, 5, p, None), 'mesh_emit', 'null')
    refused(lib.occnerf_mesh_emit(p, 4, 4, 4, 0.0, None, 5, p, None), 'mesh_emit', 'null')
    refused(lib.occnerf_mesh_emit(p, 4, 4, 4, 0.0, p, 5, None, None), 'mesh_emit', 'null')
    refused(lib.occnerf_mesh_vertices(p, 5, None, 4, 4, 4, 0.0, p, 1.0, p, None), 'mesh_vertices', 'null')
    refused(lib.occnerf_mesh_vertices(p, 5, p, 4, 4, 4, 0.0, None, 1.0, p, None), 'mesh_vertices', 'null')
    refused(lib.occnerf_mesh_vertices(None, 5, p, 4, 4, 4, 0.0, p, 1.0, p, None), 'mesh_vertices', 'null')
    refused(lib.occnerf_mesh_vertices(p, 5, p, 4, 4, 4, 0.0, p, 1.0, None, None), 'mesh_vertices', 'null')
    for shape in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (2048, 1024, 1024), (46341, 46341, 2)):
        refused(lib.occnerf_mesh_count(p, *shape, 0.0, p, None), 'mesh_count', 'bad grid')
        refused(lib.occnerf_mesh_emit(p, *shape, 0.0, p, 5, p, None), 'mesh_emit', 'bad grid')
        refused(lib.occnerf_mesh_vertices(p, 5, p, *shape, 0.0, p, 1.0, p, None), 'mesh_vertices', 'bad grid')
    refused(lib.occnerf_mesh_emit(p, 4, 4, 4, 0.0, p, -1, p, None), 'mesh_emit', 'negative')
    refused(lib.occnerf_mesh_vertices(p, -1, p, 4, 4, 4, 0.0, p, 1.0, p, None), 'mesh_vertices', 'V=-1')
    # nothing to do: 0 without a launch (there is no GPU here to launch on)
    assert lib.occnerf_mesh_emit(p, 4, 4, 4, 0.0, p, 0, None, None) == 0
    assert lib.occnerf_mesh_vertices(None, 0, p, 4, 4, 4, 0.0, p, 1.0, None, None) == 0


def test_wrappers_refuse_host_tensors():
    import torch
    from occnerf_amd import ops
    from occnerf_amd.network import Network
    field = torch.zeros(3, 3, 3)
    with pytest.raises(RuntimeError, match='field must be a CUDA'):
        ops.mesh_count(field, 0.0)
    with pytest.raises(RuntimeError, match='field must be a CUDA'):
        ops.mesh_emit(field, 0.0, torch.zeros(4, dtype=torch.int64), 0)
    with pytest.raises(RuntimeError, match='field must be a CUDA'):
        ops.mesh_vertices(torch.zeros(2, dtype=torch.int64), field, 0.0, [0, 0, 0], 1.0)
    with pytest.raises(RuntimeError, match='field must be a \\[nz,ny,nx\\]'):
        ops.mesh_count(torch.zeros(3, 3), 0.0)
    with pytest.raises(RuntimeError, match='query_canonical: xyz must be a CUDA'):
        Network.query_canonical(None, torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match='query_canonical: xyz must be a CUDA'):
        Network.query_canonical(None, np.zeros((5, 3), np.float32))


def test_run_py_names_the_mesh_type():
    src = open(os.path.join(ROOT, 'run.py')).read()
    assert 'def run_mesh():' in src and 'supported are tpose, freeview, backview, movement, allview, evaluate, mesh' in src
