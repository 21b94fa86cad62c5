"""The numpy definition of the mesh rasteriser: a triangle mesh seen through a pinhole camera as a
coverage map, the nearest triangle per pixel, its depth and its interpolated vertex colour.  csrc/mesh_raster.hip must give
these bits.

A pure function of pos [V,3] float32, faces [T,3] int32, colors [V,3] uint8, K (3x3 float64, no skew), E (4x4 float64: the
camera seen from the space pos is in), H, W and a uint8 background colour.  Floating point is float64 with + * / rint and
comparisons only, one rounding per operator in the order written here (`a + b + c` is `(a + b) + c`, nothing is fused);
everything else is integer arithmetic.

  vertex    c_k = ((R[k,0] p_0 + R[k,1] p_1) + R[k,2] p_2) + t_k with R = E[:3,:3], t = E[:3,3];
            flag 1 unless c_z >= NEAR (a NaN c_z is flag 1);  u = fx (c_x / c_z) + cx, v = fy (c_y / c_z) + cy;
            a = 256 u, b = 256 v;  flag 2 unless |a| <= GUARD and |b| <= GUARD and c_z <= FAR (NaN included);
            X = rint(a), Y = rint(b) as int32 (ties to even), z = c_z.  A flagged vertex has X = Y = 0 and z = 0.
  sample    pixel (row i, column j) is sampled at (u, v) = (j, i), in fixed point (256 j, 256 i): the integer coordinate, where
            synth.get_rays_from_KRT puts the pixel's ray, not the half-pixel centre.
  triangle  dropped, and counted under the first reason that holds: `index` a vertex index outside [0, V); `near` a vertex with
            flag 1; `guard` a vertex with flag 2; `area` A = (X1-X0)(Y2-Y0) - (Y1-Y0)(X2-X0) == 0 (int64); `offscreen` its
            bounding box misses [0, 256 (W-1)] x [0, 256 (H-1)].  Nothing is clipped.  A < 0: vertices 1 and 2 change places
            (two-sided; then A > 0).
  cover     edge functions e_0 = edge(1, 2), e_1 = edge(2, 0), e_2 = edge(0, 1) at the sample P,
            edge(a, b) = (Xb-Xa)(Py-Ya) - (Yb-Ya)(Px-Xa) in int64: |coordinate| <= 2^22 and 0 <= P <= 2^22 give differences below
            2^23, products below 2^46 and |e|, A below 2^47 -- inside int64, and exact as float64.  The sample is covered when
            every e_k > 0, or e_k == 0 on an edge with Yb - Ya < 0 (a left edge) or Yb == Ya and Xb - Xa > 0 (a top edge):
            two triangles that share an edge cover a sample on it exactly once.
  depth     q_k = (float64(e_k) / float64(A)) / z_k;  iz = (q_0 + q_1) + q_2;  depth = float32(1 / iz): perspective-correct,
            rounded once.  z_k in [NEAR, FAR] keeps it a positive finite float32.
  merge     per pixel the minimum of key = (bits of depth) << 32 | triangle index as uint64; positive floats order as their
            bits, ties go to the lower index; an empty pixel keeps the key of all ones.
  resolve   empty: cover 0, tri -1, depth +inf, rgb = background.  Else the winner's e_k, q_k and iz again at the pixel,
            w_k = q_k / iz, channel = (w_0 C_0 + w_1 C_1) + w_2 C_2 on the (re-ordered) vertices' uint8 colours,
            rgb = uint8(min(max(rint(channel), 0), 255)).
  counts    int32: the triangles dropped per reason, `wide` = the triangles whose clipped sample box holds more than WIDE
            samples (the kernels draw those in a second pass; the image does not depend on it), `covered` = pixels with cover 1.
"""
import numpy as np

NEAR = 1e-3                      # metres: a vertex nearer than a millimetre (or behind the camera) drops its triangles
FAR = 1048576.0                  # 2^20 metres
GUARD = 4194304.0                # 2^22 fixed-point units = 16 384 pixels
MAX_SIDE = 16384                 # H, W <= 2^14: 256 (W - 1) < 2^22
MAX_PIXELS = 1 << 28
WIDE = 64
COUNTS = ('index', 'near', 'guard', 'area', 'offscreen', 'wide', 'covered')
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def camera(K, E):
    """(fx, fy, cx, cy, R [3,3], t [3]) as float64; a skewed K is refused by name."""
    K, E = np.asarray(K, dtype=np.float64), np.asarray(E, dtype=np.float64)
    if K.shape != (3, 3) or E.shape != (4, 4):
        raise ValueError(f'mesh_project: K must be 3x3 and E 4x4, got {K.shape} and {E.shape}')
    if K[0, 1] != 0.0:
        raise NotImplementedError(f'mesh_project: skew K[0,1] = {K[0, 1]!r} is not built')
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2], E[:3, :3], E[:3, 3]


def project(pos, K, E):
    """-> (xy int32 [V,2], z float64 [V], vflag uint8 [V])."""
    fx, fy, cx, cy, R, t = camera(K, E)
    p = np.asarray(pos, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all='ignore'):
        c = [((R[k, 0] * p[:, 0] + R[k, 1] * p[:, 1]) + R[k, 2] * p[:, 2]) + t[k] for k in range(3)]
        near = ~(c[2] >= NEAR)
        a = 256.0 * (fx * (c[0] / c[2]) + cx)
        b = 256.0 * (fy * (c[1] / c[2]) + cy)
        out = ~((np.abs(a) <= GUARD) & (np.abs(b) <= GUARD) & (c[2] <= FAR))
        vflag = np.where(near, 1, np.where(out, 2, 0)).astype(np.uint8)
        ok = vflag == 0
        xy = np.stack([np.where(ok, np.rint(a), 0.0), np.where(ok, np.rint(b), 0.0)], 1).astype(np.int32)
    return xy, np.where(ok, c[2], 0.0), vflag


def _check_size(H, W):
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE and H * W <= MAX_PIXELS):
        raise ValueError(f'mesh_raster: H={H} W={W} outside 1..{MAX_SIDE} or more than 2^28 pixels')
    return H, W


def setup(faces, xy, vflag):
    """Per triangle: (reason int [T]: 0 kept, 1 index, 2 near, 3 guard, 4 area; idx int64 [T,3] re-ordered so that A > 0;
    A int64 [T]).  The offscreen test needs the image size and is made by the callers."""
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    V = xy.shape[0]
    bad = ((faces < 0) | (faces >= V)).any(1)
    idx = np.where(bad[:, None], 0, faces) if V else np.zeros_like(faces)
    fl = vflag[idx] if V else np.zeros(idx.shape, np.uint8)
    X, Y = (xy[idx, 0].astype(np.int64), xy[idx, 1].astype(np.int64)) if V else (idx, idx)
    A = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    reason = np.where(bad, 1, np.where((fl == 1).any(1), 2, np.where((fl == 2).any(1), 3, np.where(A == 0, 4, 0))))
    flip = A < 0
    idx = np.where(flip[:, None], idx[:, [0, 2, 1]], idx)
    return reason, idx, np.abs(A)


def edges(X, Y, Px, Py):
    """(e [3, ...] int64 at the samples, include [3] bool: an e_k == 0 counts as inside)."""
    e, inc = [], []
    for a, b in ((1, 2), (2, 0), (0, 1)):
        dx, dy = int(X[b] - X[a]), int(Y[b] - Y[a])
        e.append(dx * (Py - int(Y[a])) - dy * (Px - int(X[a])))
        inc.append(dy < 0 or (dy == 0 and dx > 0))
    return np.stack(e), inc


def inverse_depth(e, A, z3):
    """(q [3, ...], iz [...]) float64."""
    q = [(e[k].astype(np.float64) / np.float64(A)) / z3[k] for k in range(3)]
    return q, (q[0] + q[1]) + q[2]


def raster_keys(faces, xy, z, vflag, H, W):
    """-> (keys uint64 [H,W], counts dict without 'covered')."""
    H, W = _check_size(H, W)
    reason, idx, A = setup(faces, xy, vflag)
    counts = {name: int((reason == r + 1).sum()) for r, name in enumerate(COUNTS[:4])}
    counts.update(offscreen=0, wide=0)
    keys = np.full((H, W), EMPTY_KEY, dtype=np.uint64)
    kept = np.nonzero(reason == 0)[0]
    if kept.size:                                     # the boxes of all kept triangles at once; the loop visits the rest
        X, Y = xy[idx[kept], 0].astype(np.int64), xy[idx[kept], 1].astype(np.int64)
        off = (X.max(1) < 0) | (X.min(1) > 256 * (W - 1)) | (Y.max(1) < 0) | (Y.min(1) > 256 * (H - 1))
        counts['offscreen'] = int(off.sum())
        j0, j1 = np.maximum(0, (X.min(1) + 255) >> 8), np.minimum(W - 1, X.max(1) >> 8)
        i0, i1 = np.maximum(0, (Y.min(1) + 255) >> 8), np.minimum(H - 1, Y.max(1) >> 8)
        n = np.where(off, 0, np.maximum(j1 - j0 + 1, 0) * np.maximum(i1 - i0 + 1, 0))
        counts['wide'] = int((n > WIDE).sum())
        for k in np.nonzero(n > 0)[0]:
            t = int(kept[k])
            Px, Py = np.meshgrid(256 * np.arange(j0[k], j1[k] + 1, dtype=np.int64), 256 * np.arange(i0[k], i1[k] + 1, dtype=np.int64))
            e, inc = edges(X[k], Y[k], Px, Py)
            cov = np.ones(Px.shape, dtype=bool)
            for m in range(3):
                cov &= (e[m] > 0) | ((e[m] == 0) & inc[m])
            if not cov.any():
                continue
            _, iz = inverse_depth(e[:, cov], A[t], z[idx[t]])
            depth = (1.0 / iz).astype(np.float32)
            key = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
            view = keys[i0[k]:i1[k] + 1, j0[k]:j1[k] + 1]
            view[cov] = np.minimum(view[cov], key)
    return keys, counts


def resolve(keys, faces, xy, z, vflag, colors, bgcolor):
    """-> (cover uint8 [H,W], tri int32 [H,W], depth float32 [H,W], rgb uint8 [H,W,3], covered int)."""
    H, W = keys.shape
    _, idx, A = setup(faces, xy, vflag)
    colors = np.asarray(colors, dtype=np.uint8).reshape(-1, 3)
    hit = keys != EMPTY_KEY
    tri = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32), np.uint32(0x7F800000)).astype(np.uint32).view(np.float32)
    rgb = np.empty((H, W, 3), dtype=np.uint8)
    rgb[:] = np.asarray(bgcolor, dtype=np.uint8).reshape(3)
    for i, j in zip(*np.nonzero(hit)):
        t = int(tri[i, j])
        v = idx[t]
        e, _ = edges(xy[v, 0].astype(np.int64), xy[v, 1].astype(np.int64), np.int64(256 * j), np.int64(256 * i))
        q, iz = inverse_depth(e, A[t], z[v])
        w = [q[k] / iz for k in range(3)]
        c = colors[v].astype(np.float64)
        s = (w[0] * c[0] + w[1] * c[1]) + w[2] * c[2]
        rgb[i, j] = np.minimum(np.maximum(np.rint(s), 0.0), 255.0).astype(np.uint8)
    return hit.astype(np.uint8), tri, depth, rgb, int(hit.sum())


def rasterize(pos, faces, colors, K, E, H, W, bgcolor=(255, 255, 255)):
    """The whole definition -> a dict: xy, z, vflag, keys, cover, tri, depth, rgb and counts (a dict over COUNTS)."""
    xy, z, vflag = project(pos, K, E)
    keys, counts = raster_keys(faces, xy, z, vflag, H, W)
    cover, tri, depth, rgb, covered = resolve(keys, faces, xy, z, vflag, colors, bgcolor)
    counts['covered'] = covered
    return {'xy': xy, 'z': z, 'vflag': vflag, 'keys': keys, 'cover': cover, 'tri': tri, 'depth': depth, 'rgb': rgb,
            'counts': counts}


def count_vector(counts):
    return np.array([counts[k] for k in COUNTS], dtype=np.int32)


def mask_iou(cover, gt_alpha):
    """(intersection, union, IoU or None, covered, share of the covered pixels inside the mask or None): the silhouette
    against gt_alpha > 0.5, the threshold eval.py takes for the ground-truth silhouette; exact integers, IoU = I / U in float64."""
    a, b = np.asarray(cover) > 0, np.asarray(gt_alpha) > 0.5
    inter, union, covered = int((a & b).sum()), int((a | b).sum()), int(a.sum())
    return inter, union, (inter / union if union else None), covered, (inter / covered if covered else None)


# ------------------------------------------------------------------ the cases the CPU and the GPU tests share
def pinhole(H, W, focal=None, cz=3.0):
    """A camera looking along +z of the mesh's space from cz behind its origin: K with the principal point at the image centre,
    E a pure translation."""
    f = float(focal if focal is not None else 0.9 * max(H, W))
    K = np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])
    E = np.eye(4)
    E[2, 3] = cz
    return K, E


def unproject(K, E, uv, depth):
    """float32 [n,3] points of E's source space that the camera (K, E) sees at pixel position uv [n,2] at depth [n] (they
    land there up to their float32 rounding)."""
    uv, depth = np.asarray(uv, dtype=np.float64), np.asarray(depth, dtype=np.float64)
    cam = np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0] * depth, (uv[:, 1] - K[1, 2]) / K[1, 1] * depth, depth], 1)
    return ((cam - E[:3, 3]) @ E[:3, :3]).astype(np.float32)


def grid_mesh(nx, ny):
    """(uv-grid indices [ (ny+1)(nx+1), 2 ], faces): a regular grid of nx x ny cells, each split into two triangles, the
    diagonal alternating from cell to cell, with mixed windings."""
    gy, gx = np.mgrid[0:ny + 1, 0:nx + 1]
    g = np.stack([gx.ravel(), gy.ravel()], 1)
    faces = []
    for y in range(ny):
        for x in range(nx):
            a, b, c, d = y * (nx + 1) + x, y * (nx + 1) + x + 1, (y + 1) * (nx + 1) + x, (y + 1) * (nx + 1) + x + 1
            if (x + y) % 2:
                faces += [[a, b, d], [a, c, d]]          # the second is wound the other way
            else:
                faces += [[a, b, c], [d, c, b]]
    return g, np.array(faces, dtype=np.int32)


def vertex_colors(n, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (n, 3)).astype(np.uint8)


def case_grid(H=48, W=64, cell=8):
    """Triangles whose shared edges and vertices pass exactly through samples: grid vertices on whole pixels, every `cell`-th
    pixel, at depths that vary from vertex to vertex; the projection is set up in exact arithmetic (K, E = I, powers of two),
    so the fixed-point vertices are 256 x those pixels exactly.  cell 8: every triangle's box holds 81 samples (the wide
    pass); cell 4: 25 (the narrow pass)."""
    g, faces = grid_mesh(48 // cell, 32 // cell)
    uv = g * float(cell) + 4.0                                # columns 4..52, rows 4..36
    depth = 2.0 + ((g[:, 0] * 3 + g[:, 1] * 5) % 4) * 0.5   # 2, 2.5, 3, 3.5: exact
    K = np.array([[64.0, 0.0, 0.0], [0.0, 64.0, 0.0], [0.0, 0.0, 1.0]])
    pos = np.stack([uv[:, 0] / 64.0 * depth, uv[:, 1] / 64.0 * depth, depth], 1).astype(np.float32)
    return {'pos': pos, 'faces': faces, 'colors': vertex_colors(len(pos), 1), 'K': K, 'E': np.eye(4), 'H': H, 'W': W,
            'uv': uv}


def case_grid4(H=48, W=64):
    return case_grid(H, W, cell=4)


def case_flags(H=48, W=64):
    """One triangle per reason, and two that stay: [0] behind the near plane, [1] past the guard band, [2] zero area (a
    repeated vertex), [3] zero area (collinear in fixed point), [4] wholly off screen, [5] partly off screen (kept, not
    clipped), [6] wholly inside, [7] an index outside [0, V)."""
    K, E = pinhole(H, W)
    uv = np.array([[10, 10], [20, 10], [10, 20],              # 0: vertex 2 gets depth behind the camera
                   [30, 10], [40, 10], [1e6, 20],              # 1: vertex 5 far outside the guard band
                   [5, 30], [15, 30], [15, 40],                # 2: faces use vertex 6 twice
                   [20, 30], [24, 34], [28, 38],               # 3: collinear
                   [-40, 5], [-30, 5], [-35, 15],              # 4: left of the image
                   [50, 20], [90, 25], [55, 44],               # 5: crosses the right border
                   [30, 22], [44, 26], [33, 40]], dtype=np.float64)     # 6
    depth = np.full(len(uv), 3.0)
    pos = unproject(K, E, uv, depth)
    pos[2] = unproject(K, E, uv[2:3], [1.0])[0]
    pos[2, 2] = -E[2, 3] + 0.0005                              # c_z = 0.0005 < NEAR
    faces = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 6], [9, 10, 11], [12, 13, 14], [15, 16, 17], [18, 19, 20], [0, 1, 21]],
                     dtype=np.int32)
    return {'pos': pos, 'faces': faces, 'colors': vertex_colors(len(pos), 2), 'K': K, 'E': E, 'H': H, 'W': W}


def case_ties(H=48, W=64):
    """Triangles 0 and 1 coincide (the lower index wins), triangle 2 lies nearer over a part of them and wins there, triangle 3
    lies farther and is hidden where they are."""
    K, E = pinhole(H, W)
    big = np.array([[8, 6], [56, 10], [20, 42]], dtype=np.float64)
    small = np.array([[16, 12], [40, 14], [22, 30]], dtype=np.float64)
    far = np.array([[4, 4], [60, 6], [30, 46]], dtype=np.float64)
    pos = np.concatenate([unproject(K, E, big, [3.0, 3.2, 3.4]), unproject(K, E, small, [2.0, 2.1, 2.2]),
                          unproject(K, E, far, [5.0, 5.0, 5.5])])
    faces = np.array([[0, 1, 2], [2, 0, 1], [3, 4, 5], [6, 7, 8]], dtype=np.int32)
    return {'pos': pos, 'faces': faces, 'colors': vertex_colors(len(pos), 3), 'K': K, 'E': E, 'H': H, 'W': W}


def case_mixed(H=80, W=96, n_small=300, seed=4):
    """Two triangles filling the image at depth 4 (the wide pass), a few hundred small ones (the narrow pass) at depths 2..6
    scattered over it: in front of and behind the large ones, so both passes write the same pixels."""
    K, E = pinhole(H, W)
    rng = np.random.RandomState(seed)
    corners = np.array([[-2, -2], [W + 2, -2], [-2, H + 2], [W + 2, H + 2]], dtype=np.float64)
    big = unproject(K, E, corners, np.full(4, 4.0))
    centre = rng.uniform([2, 2], [W - 3, H - 3], (n_small, 2))
    tri_uv = centre[:, None, :] + rng.uniform(-2.5, 2.5, (n_small, 3, 2))
    d = rng.uniform(2.0, 6.0, n_small)
    small = unproject(K, E, tri_uv.reshape(-1, 2), np.repeat(d, 3) + rng.uniform(-0.05, 0.05, 3 * n_small))
    pos = np.concatenate([big, small])
    faces = np.concatenate([[[0, 1, 2], [3, 2, 1]], 4 + np.arange(3 * n_small).reshape(-1, 3)]).astype(np.int32)
    order = rng.permutation(len(faces))                      # the large ones somewhere among the small
    return {'pos': pos, 'faces': np.ascontiguousarray(faces[order]), 'colors': vertex_colors(len(pos), 5), 'K': K, 'E': E,
            'H': H, 'W': W}


def case_offscreen(H=48, W=64, n=40, seed=6):
    """Every triangle right of or below the image."""
    K, E = pinhole(H, W)
    rng = np.random.RandomState(seed)
    uv = rng.uniform([W + 5, H + 5], [W + 60, H + 60], (3 * n, 2))
    return {'pos': unproject(K, E, uv, rng.uniform(2.0, 4.0, 3 * n)), 'faces': np.arange(3 * n, dtype=np.int32).reshape(-1, 3),
            'colors': vertex_colors(3 * n, 7), 'K': K, 'E': E, 'H': H, 'W': W}


def case_blobs(H=48, W=64, n=24, seed=8):
    """Triangles many pixels wide at random depths, overlapping: the mesh of the independent judge of coverage and depth."""
    K, E = pinhole(H, W)
    rng = np.random.RandomState(seed)
    centre = rng.uniform([4, 4], [W - 5, H - 5], (n, 2))
    uv = centre[:, None, :] + rng.uniform(-14, 14, (n, 3, 2))
    return {'pos': unproject(K, E, uv.reshape(-1, 2), rng.uniform(2.0, 5.0, 3 * n)),
            'faces': np.arange(3 * n, dtype=np.int32).reshape(-1, 3), 'colors': vertex_colors(3 * n, 9), 'K': K, 'E': E,
            'H': H, 'W': W}


def case_random(T, H=48, W=64, seed=10):
    """T triangles of a few pixels each over a shared pool of vertices (T = 0 included)."""
    K, E = pinhole(H, W)
    rng = np.random.RandomState(seed + T)
    V = max(3, T // 2 + 3)
    uv = rng.uniform([-4, -4], [W + 4, H + 4], (V, 2))
    pos = unproject(K, E, uv, rng.uniform(2.0, 4.0, V))
    first = rng.randint(0, V, T)
    near = np.argsort(((uv[first][:, None, :] - uv[None, :, :]) ** 2).sum(-1), axis=1)[:, :3] if T else np.zeros((0, 3), np.int64)
    return {'pos': pos, 'faces': near.astype(np.int32).reshape(-1, 3), 'colors': vertex_colors(V, 11), 'K': K, 'E': E, 'H': H, 'W': W}


CASES = {'grid': case_grid, 'grid4': case_grid4, 'flags': case_flags, 'ties': case_ties, 'mixed': case_mixed, 'offscreen': case_offscreen,
         'blobs': case_blobs}


def run_case(c, **kw):
    return rasterize(c['pos'], c['faces'], c['colors'], c['K'], c['E'], kw.get('H', c['H']), kw.get('W', c['W']),
                     kw.get('bgcolor', (255, 255, 255)))


# ------------------------------------------------------------------ the posed SyntheticSMPL mesh in a tool-made dataset
def load_tool():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('make_synthetic_dataset', os.path.join(root, 'tools', 'make_synthetic_dataset.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def posed_smpl(tool, info):
    """(posed float32 [6890,3] in the body's own space by the tool's forward kinematics, faces int32 [13 684,3], colours)."""
    from occnerf_amd import synth
    model = synth.SyntheticSMPL()
    verts, _ = model(np.zeros(72), info['betas'])
    posed, _ = tool.posed_body(info['poses'].astype(np.float64), info['tpose_joints'].astype(np.float64), verts,
                               tool.vertex_joints())
    return posed.astype(np.float32), np.asarray(model.faces, dtype=np.int32), tool.vertex_colours(verts)
