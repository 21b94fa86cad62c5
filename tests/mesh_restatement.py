"""The numpy definition of the mesh extraction, written from the definition alone: marching
tetrahedra on the Kuhn split of every cube of a [nz, ny, nx] float32 field.

  * cube corner c = dx + 2 dy + 4 dz; tetrahedron t of a cube (t = 0..5, the permutations of the axes (x, y, z) in
    lexicographic order) has the corners 0, e_p0, e_p0 + e_p1, 7: all six share the body diagonal 0 -> 7;
  * a corner is inside iff f > level, compared in float32 (NaN is outside);
  * a surface vertex lies on an edge that leaves a grid point `lo` in a non-negative direction d != 0; its name is the
    int64 key lo_linear * 7 + (dx + 2 dy + 4 dz - 1), lo_linear = (z * ny + y) * nx + x;
  * the triangles come out in the order (z, y, x, tetrahedron, triangle within the case), wound so that (b - a) x (c - a)
    points from the inside corners to the outside ones (CASE_TABLE, built below from the geometry of the unit cube);
  * welding is np.unique over the keys; a vertex is pa + t (pb - pa) in grid coordinates with t = (level - fa) / (fb - fa)
    in float64, one rounding per operator, then min + p * h rounded once to float32.  A t outside [0, 1] (NaN included:
    only non-finite end values produce one) is replaced by 0.5.
"""
import itertools

import numpy as np

PERMS = list(itertools.permutations(range(3)))
EMPTY = 0xFF


def tet_corners(t):
    """The four cube corners of tetrahedron t, along its path from corner 0 to corner 7."""
    c = [0]
    for axis in PERMS[t]:
        c.append(c[-1] | (1 << axis))
    return c


def _corner_xyz(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)


def _case_triangles(t, m):
    """Triangles of tetrahedron t whose vertex i is inside iff bit i of m is set: a list of triangles, each three tetrahedron
    edges (i, j), i < j, wound by the geometry of the edge midpoints."""
    cs = tet_corners(t)
    pos = [_corner_xyz(c) for c in cs]
    inside = [i for i in range(4) if (m >> i) & 1]
    outside = [i for i in range(4) if not (m >> i) & 1]
    e = lambda i, j: (min(i, j), max(i, j))          # noqa: E731
    if len(inside) in (0, 4):
        return []
    if len(inside) == 1 or len(outside) == 1:
        a = inside[0] if len(inside) == 1 else outside[0]
        b, c, d = outside if len(inside) == 1 else inside
        tris = [[e(a, b), e(a, c), e(a, d)]]
    else:
        a, b = inside
        c, d = outside
        tris = [[e(a, c), e(a, d), e(b, d)], [e(a, c), e(b, d), e(b, c)]]
    want = np.mean([pos[i] for i in outside], axis=0) - np.mean([pos[i] for i in inside], axis=0)
    out = []
    for tri in tris:
        q = [(pos[i] + pos[j]) / 2 for i, j in tri]
        s = float(np.dot(np.cross(q[1] - q[0], q[2] - q[0]), want))
        assert s != 0.0
        out.append(tri if s > 0 else [tri[0], tri[2], tri[1]])
    return out


def edge_code(t, i, j):
    """corner * 8 + kind of the edge (i, j) of tetrahedron t: the cube corner its lo end sits on, and its direction."""
    cs = tet_corners(t)
    return cs[i] * 8 + (cs[j] - cs[i] - 1)


def case_table():
    """uint8 [6, 16, 6]: per tetrahedron and inside mask, the edge codes of up to two triangles, EMPTY where there is none."""
    tab = np.full((6, 16, 6), EMPTY, dtype=np.uint8)
    for t in range(6):
        for m in range(16):
            for k, tri in enumerate(_case_triangles(t, m)):
                for v, (i, j) in enumerate(tri):
                    tab[t, m, 3 * k + v] = edge_code(t, i, j)
    return tab


CASE_TABLE = case_table()


def extract_keys(field, level):
    """-> (row_count int32 [(nz-1)*(ny-1)], tri_keys int64 [T,3]) in the stated order."""
    f = np.asarray(field, dtype=np.float32)
    nz, ny, nx = f.shape
    assert min(nx, ny, nz) >= 2
    with np.errstate(invalid='ignore'):
        inside = f > np.float32(level)
    cz, cy, cx = nz - 1, ny - 1, nx - 1

    def corner(c):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        return inside[dz:dz + cz, dy:dy + cy, dx:dx + cx]
    zz, yy, xx = np.meshgrid(np.arange(cz), np.arange(cy), np.arange(cx), indexing='ij')
    lin = ((zz * ny + yy) * nx + xx).astype(np.int64).ravel()
    keys, order = [], []
    for t in range(6):
        cs = tet_corners(t)
        mask = sum(corner(cs[i]).astype(np.int64) << i for i in range(4)).ravel()
        for m in range(1, 15):
            cubes = np.nonzero(mask == m)[0]
            if cubes.size == 0:
                continue
            for k in range(2):
                codes = CASE_TABLE[t, m, 3 * k:3 * k + 3]
                if codes[0] == EMPTY:
                    continue
                tri = np.empty((cubes.size, 3), dtype=np.int64)
                for v, code in enumerate(int(c) for c in codes):
                    c, kind = code >> 3, code & 7
                    off = (c & 1) + ((c >> 1) & 1) * nx + ((c >> 2) & 1) * nx * ny
                    tri[:, v] = (lin[cubes] + off) * 7 + kind
                keys.append(tri)
                order.append((cubes * 6 + t) * 2 + k)
    if not keys:
        return np.zeros(cz * cy, dtype=np.int32), np.zeros((0, 3), dtype=np.int64)
    keys, order = np.concatenate(keys), np.concatenate(order)
    by = np.argsort(order, kind='stable')
    rows = order[by] // (12 * cx)
    return np.bincount(rows, minlength=cz * cy).astype(np.int32), keys[by]


def weld(tri_keys):
    """-> (vertex keys ascending int64 [V], faces int32 [T,3])."""
    vkeys, inv = np.unique(np.asarray(tri_keys, dtype=np.int64).reshape(-1), return_inverse=True)
    return vkeys, inv.reshape(-1, 3).astype(np.int32)


def vertices(vkeys, field, level, bbox_min, h):
    """float32 [V,3] world positions of the keyed vertices."""
    f = np.asarray(field, dtype=np.float32)
    nz, ny, nx = f.shape
    vkeys = np.asarray(vkeys, dtype=np.int64)
    lo, kind = vkeys // 7, vkeys % 7 + 1
    d = np.stack([kind & 1, (kind >> 1) & 1, (kind >> 2) & 1], axis=1)
    a = np.stack([lo % nx, lo // nx % ny, lo // (nx * ny)], axis=1)
    flat = f.reshape(-1)
    fa = flat[lo].astype(np.float64)
    fb = flat[lo + d[:, 0] + d[:, 1] * nx + d[:, 2] * nx * ny].astype(np.float64)
    with np.errstate(all='ignore'):
        t = (np.float64(np.float32(level)) - fa) / (fb - fa)
        t = np.where((t >= 0.0) & (t <= 1.0), t, 0.5)
    p = a.astype(np.float64) + t[:, None] * d.astype(np.float64)
    world = np.asarray(bbox_min, dtype=np.float64)[None, :] + p * np.float64(h)
    return world.astype(np.float32)


def extract_mesh(field, level, bbox_min, h):
    """-> (verts float32 [V,3], faces int32 [T,3])."""
    _, tri_keys = extract_keys(field, level)
    vkeys, faces = weld(tri_keys)
    return vertices(vkeys, field, level, bbox_min, h), faces


# ------------------------------------------------------------------ fields and checks the tests share
def random_fields():
    """The 20 seeded 5 x 6 x 7-point fields of normal deviates whose boundary layer is forced to -1 (level 0: no ties)."""
    out = []
    for seed in range(20):
        f = np.random.RandomState(100 + seed).randn(7, 6, 5).astype(np.float32)
        f[0] = f[-1] = f[:, 0] = f[:, -1] = f[:, :, 0] = f[:, :, -1] = -1.0
        out.append(f)
    return out


def sphere_field(n=17, radius=5.3):
    g = np.arange(n, dtype=np.float64)
    z, y, x = np.meshgrid(g, g, g, indexing='ij')
    c = (n - 1) / 2 + 0.13
    return (radius - np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)).astype(np.float32), np.array([c, c, c])


def torus_field(n=17, major=4.6, minor=1.9):
    g = np.arange(n, dtype=np.float64)
    z, y, x = np.meshgrid(g, g, g, indexing='ij')
    c = (n - 1) / 2 + 0.13
    ring = np.sqrt((x - c) ** 2 + (y - c) ** 2) - major
    return (minor - np.sqrt(ring ** 2 + (z - c) ** 2)).astype(np.float32)


def edge_value_field():
    """A closed blob with one corner exactly at the level (outside) and one NaN corner (outside) next to inside points."""
    f, _ = sphere_field(9, 2.6)
    f[4, 4, 6] = np.float32(0.0)          # was inside (distance 2 from the centre): now exactly the level
    f[4, 6, 4] = np.float32(np.nan)
    return f


def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed(faces):
    """Every undirected edge lies in exactly two triangles, once in each direction (exact integer check)."""
    e = directed_edges(faces)
    if e.shape[0] == 0:
        return True
    n = int(e.max()) + 1
    fwd = np.sort(e[:, 0] * n + e[:, 1])
    bwd = np.sort(e[:, 1] * n + e[:, 0])
    return bool(np.unique(fwd).size == fwd.size and np.array_equal(fwd, bwd))


def euler_characteristic(n_verts, faces):
    e = np.sort(directed_edges(faces), axis=1)
    return int(n_verts) - int(np.unique(e, axis=0).shape[0]) + int(np.asarray(faces).shape[0])


def signed_volume(verts, faces):
    v = np.asarray(verts, dtype=np.float64)[np.asarray(faces)]
    return float(np.einsum('ij,ij->i', v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def parse_ply(data):
    """A binary little-endian PLY as occnerf_amd.mesh.write_ply writes it -> dict of its vertex properties and 'faces'."""
    head, _, body = data.partition(b'end_header\n')
    lines = head.decode('ascii').split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0'
    nv = nf = 0
    props, elem = [], None
    for ln in lines[2:]:
        w = ln.split()
        if not w or w[0] == 'comment':
            continue
        if w[0] == 'element':
            elem = w[1]
            if elem == 'vertex':
                nv = int(w[2])
            else:
                assert elem == 'face'
                nf = int(w[2])
        elif w[0] == 'property' and elem == 'vertex':
            props.append((w[2], {'float': '<f4', 'uchar': 'u1'}[w[1]]))
        elif w[0] == 'property':
            assert w[1:] == ['list', 'uchar', 'int', 'vertex_indices']
    vt = np.dtype(props)
    ft = np.dtype([('n', 'u1'), ('v', '<i4', (3,))])
    assert len(body) == nv * vt.itemsize + nf * ft.itemsize
    v = np.frombuffer(body, dtype=vt, count=nv)
    fc = np.frombuffer(body, dtype=ft, count=nf, offset=nv * vt.itemsize)
    assert (fc['n'] == 3).all()
    out = {name: v[name] for name, _ in props}
    out['faces'] = fc['v']
    return out
