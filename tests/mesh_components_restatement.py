"""The numpy definition of the mesh clean-up, written from the definition alone: connected components
of a welded triangle mesh, their integer records, the selection and the filter.

  * two triangles are connected when they share a vertex index; a component is a set of vertices and its label is the
    smallest vertex index in it; a vertex no face names is a component of its own with 0 triangles; a degenerate face
    connects what it names and counts as a triangle; components are listed in ascending label order;
  * labels: from labels[v] = v, synchronous rounds -- every triangle's smallest label is written (minimum) into its three
    vertices, then labels = labels[labels] -- until a round changes nothing;
  * snapped coordinates s = rint(((float64(v) - lo) / h) * 1024) per axis, one rounding per operator, held to [-2^30, 2^30]
    (NaN: the lower end); a vertex is a boundary vertex when some s[a] is 0 or (n[a] - 1) * 1024;
  * the record of a component: vertices, triangles (a triangle belongs to the component of its first vertex),
    boundary_vertices, smin[3], smax[3] and volume6_q = the sum over its triangles of
    det = a_x (b_y c_z - b_z c_y) + a_y (b_z c_x - b_x c_z) + a_z (b_x c_y - b_y c_x) in int64 with wrap-around;
  * a component is a cavity when boundary_vertices == 0 and volume6_q < 0;
  * selection: 'all', 'largest' (the most triangles; ties: the smaller label) or f in (0, 1] (triangles >= f * the largest
    count, in float64), then drop_cavities among what the size rule kept;
  * filter: kept vertices in their order, kept triangles in theirs, indices remapped by the exclusive scan of the keep flags.
"""
import numpy as np

SNAP = 1024
LIMIT = float(1 << 30)


def labels(faces, n_verts, rounds=None):
    """int32 [V]; rounds: a list that receives the number of rounds taken (the last one changes nothing)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    lab = np.arange(int(n_verts), dtype=np.int64)
    assert f.size == 0 or (f.min() >= 0 and f.max() < n_verts)
    n = 0
    while True:
        n += 1
        new = lab.copy()
        if f.size:
            m = lab[f].min(axis=1)
            np.minimum.at(new, f.reshape(-1), np.repeat(m, 3))
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    if rounds is not None:
        rounds.append(n)
    return lab.astype(np.int32)


def snapped(verts, bbox_min, h):
    """int64 [V,3]."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    lo = np.asarray(bbox_min, dtype=np.float64).reshape(3)
    with np.errstate(all='ignore'):
        q = ((v - lo[None, :]) / np.float64(h)) * np.float64(SNAP)
        q = np.where(q >= -LIMIT, q, -LIMIT)
        q = np.where(q > LIMIT, LIMIT, q)
    return np.rint(q).astype(np.int64)


def records(verts, faces, lab, bbox_min, h, shape):
    """dict of arrays, one row per component in ascending label order."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    lab = np.asarray(lab, dtype=np.int64)
    V = lab.shape[0]
    roots = np.nonzero(lab == np.arange(V))[0]
    C = roots.shape[0]
    rank_of = np.full(V, -1, dtype=np.int64)
    rank_of[roots] = np.arange(C)
    vrank = rank_of[lab]
    s = snapped(verts, bbox_min, h)
    edge = (np.asarray(shape, dtype=np.int64).reshape(3) - 1) * SNAP
    on_boundary = ((s == 0) | (s == edge[None, :])).any(axis=1)
    rec = {'label': roots.astype(np.int32), 'vertices': np.zeros(C, np.int64), 'triangles': np.zeros(C, np.int64),
           'boundary_vertices': np.zeros(C, np.int64), 'smin': np.full((C, 3), np.iinfo(np.int32).max, np.int64),
           'smax': np.full((C, 3), np.iinfo(np.int32).min, np.int64), 'volume6_q': np.zeros(C, np.int64)}
    np.add.at(rec['vertices'], vrank, 1)
    np.add.at(rec['boundary_vertices'], vrank, on_boundary.astype(np.int64))
    for a in range(3):
        np.minimum.at(rec['smin'][:, a], vrank, s[:, a])
        np.maximum.at(rec['smax'][:, a], vrank, s[:, a])
    if f.shape[0]:
        a, b, c = s[f[:, 0]], s[f[:, 1]], s[f[:, 2]]
        with np.errstate(over='ignore'):
            det = a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) + a[:, 1] * (b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]) + \
                a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])
            trank = vrank[f[:, 0]]
            np.add.at(rec['triangles'], trank, 1)
            np.add.at(rec['volume6_q'], trank, det)
    for k in ('vertices', 'triangles', 'boundary_vertices', 'smin', 'smax'):
        rec[k] = rec[k].astype(np.int32)
    return rec


def is_cavity(rec):
    return (rec['boundary_vertices'] == 0) & (rec['volume6_q'] < 0)


def select(rec, components='all', drop_cavities=False):
    """bool [C]."""
    tri = np.asarray(rec['triangles'], dtype=np.int64)
    C = tri.shape[0]
    if isinstance(components, str):
        assert components in ('all', 'largest'), components
        keep = np.ones(C, dtype=bool)
        if components == 'largest' and C:
            keep[:] = False
            keep[int(np.argmax(tri))] = True           # the first of equals: the smaller label
    else:
        f = float(components)
        assert 0.0 < f <= 1.0
        keep = tri.astype(np.float64) >= np.float64(f) * np.float64(tri.max() if C else 0)
    if drop_cavities:
        keep = keep & ~is_cavity(rec)
    return keep


def filter_mesh(verts, faces, lab, keep):
    """(verts [V',3], faces int32 [T',3]): keep = bool per component in ascending label order."""
    verts = np.asarray(verts)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    lab = np.asarray(lab, dtype=np.int64)
    roots = np.nonzero(lab == np.arange(lab.shape[0]))[0]
    keep_label = np.zeros(lab.shape[0], dtype=bool)
    keep_label[roots] = np.asarray(keep, dtype=bool)
    keep_v = keep_label[lab]
    new_index = np.cumsum(keep_v) - keep_v                 # exclusive scan
    keep_t = keep_v[f[:, 0]] if f.shape[0] else np.zeros(0, dtype=bool)
    return verts[keep_v], new_index[f[keep_t]].astype(np.int32).reshape(-1, 3)


def components(verts, faces, bbox_min, h, shape):
    lab = labels(faces, np.asarray(verts).reshape(-1, 3).shape[0])
    return lab, records(verts, faces, lab, bbox_min, h, shape)


def volume(rec, h=1.0):
    """The signed volume of every component, in the cube of h's unit."""
    return rec['volume6_q'].astype(np.float64) * (np.float64(h) / SNAP) ** 3 / 6.0


def volume_snap_bound(verts, faces, bbox_min, h):
    """A bound on |volume from the snapped coordinates - volume from the float64 ones| of the triangles `faces`, in voxels^3,
    from the snapping alone: every coordinate moves by at most d = 1/2048 voxel (+ the float64 roundings of the quotient, 1e-12
    here).  det is linear in every row, so the change of sum det / 6 is
      first order   sum over vertices of g_v . dv,  g_v = (1/6) the sum over the triangles at v of the cross product of the
                    other two vertices in cyclic order:  <= d * sum_v |g_v|_1;
      second order  three terms det(da, db, c) per triangle, each <= |da| |db| |c| <= 3 d^2 |c|;
      third order   det(da, db, dc) <= (sqrt 3 d)^3."""
    p = (np.asarray(verts, dtype=np.float64) - np.asarray(bbox_min, dtype=np.float64)[None, :]) / float(h)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    d = 1.0 / 2048 + 1e-12
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    g = np.zeros_like(p)
    np.add.at(g, f[:, 0], np.cross(b, c))
    np.add.at(g, f[:, 1], np.cross(c, a))
    np.add.at(g, f[:, 2], np.cross(a, b))
    first = d * np.abs(g).sum() / 6.0
    norms = np.linalg.norm(a, axis=1) + np.linalg.norm(b, axis=1) + np.linalg.norm(c, axis=1)
    second = (3 * d * d * norms).sum() / 6.0
    third = f.shape[0] * (np.sqrt(3.0) * d) ** 3 / 6.0
    return float(first + second + third) * (1 + 1e-9)


# ------------------------------------------------------------------ fields and meshes the tests share
def shell_field(n=21, mid=6.2, half=2.1):
    """Matter for mid - half < r < mid + half around the centre of an n^3 grid: an outer surface and a cavity."""
    g = np.arange(n, dtype=np.float64)
    z, y, x = np.meshgrid(g, g, g, indexing='ij')
    c = (n - 1) / 2
    r = np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)
    return (half - np.abs(r - mid)).astype(np.float32)


def shell_floater_field():
    """The shell and a ball of radius 1.6 at (2.5, 2.5, 2.5), which comes first in the vertex order."""
    f = shell_field()
    g = np.arange(f.shape[0], dtype=np.float64)
    z, y, x = np.meshgrid(g, g, g, indexing='ij')
    ball = 1.6 - np.sqrt((x - 2.5) ** 2 + (y - 2.5) ** 2 + (z - 2.5) ** 2)
    return np.maximum(f, ball.astype(np.float32))


def clipped_sphere_field(n=13, radius=4.2):
    """A ball centred on the grid's x = 0 face: the surface meets the boundary and is open there."""
    g = np.arange(n, dtype=np.float64)
    z, y, x = np.meshgrid(g, g, g, indexing='ij')
    c = (n - 1) / 2
    return (radius - np.sqrt(x ** 2 + (y - c) ** 2 + (z - c) ** 2)).astype(np.float32)


def rod_field():
    """-1 on 5 x 5 x 200 points (x, y, z) with +1 on the inner axis: one closed component, 200 cubes long."""
    f = -np.ones((200, 5, 5), dtype=np.float32)
    f[1:-1, 2, 2] = 1.0
    return f


def disjoint_triangles(n=3000, seed=3):
    """n triangles without a shared vertex and 7 vertices no face names; the vertex indices are shuffled."""
    rng = np.random.RandomState(seed)
    V = 3 * n + 7
    perm = rng.permutation(V)
    faces = perm[:3 * n].reshape(n, 3).astype(np.int32)
    verts = rng.uniform(0.5, 9.5, (V, 3)).astype(np.float32)
    return verts, faces


def partition(lab):
    """The components as a canonical value that does not depend on the numbering: the sorted vertex sets' sizes."""
    _, counts = np.unique(np.asarray(lab), return_counts=True)
    return np.sort(counts)
