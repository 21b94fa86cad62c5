"""The skeleton panel's definition in numpy: what csrc/skeleton.hip must equal byte for byte.

Everything is float64 with one rounding per written operator: no dot, @ or einsum (a BLAS may fuse a product into a sum),
the parentheses are the order of evaluation.  Vectorised over the pixels, a Python loop over the 47 primitives."""
import numpy as np

JOINTS = 24
BONES = JOINTS - 1
PRIMS = BONES + JOINTS
PARENT = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)       # SMPL's tree


def project(joints, K, E):
    """-> (u, v, z float64 [24], ok bool [24]): the camera point c = ((E_r0 x + E_r1 y) + E_r2 z) + E_r3 per row r, then
    u = (K00 c_0) / c_2 + K02 and v = (K11 c_1) / c_2 + K12.  ok: every one of c, u, v is finite and c_2 > 0."""
    K, E = np.asarray(K, dtype=np.float64)[:3, :3], np.asarray(E, dtype=np.float64)
    if K[0, 1] != 0.0:
        raise NotImplementedError(f'skeleton panel: skew K[0,1] = {K[0, 1]!r} is not built')
    j = np.asarray(joints)
    assert j.shape == (JOINTS, 3) and j.dtype == np.float32, (j.shape, j.dtype)
    x, y, z = (j[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all='ignore'):
        c = [((E[r, 0] * x + E[r, 1] * y) + E[r, 2] * z) + E[r, 3] for r in range(3)]
        u = (K[0, 0] * c[0]) / c[2] + K[0, 2]
        v = (K[1, 1] * c[1]) / c[2] + K[1, 2]
        ok = np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2]) & (c[2] > 0.0) & np.isfinite(u) & np.isfinite(v)
    return u, v, c[2], ok


def primitives(joints, K, E, bone_px):
    """The 47 primitives in index order: 23 bones (bone q joins joint a = q + 1 and its parent b; radius bone_px; key
    (z_a + z_b) * 0.5; colour index a), then 24 discs (radius 1.5 * bone_px; key z; colour index the joint)."""
    u, v, z, ok = project(joints, K, E)
    r = np.float64(bone_px)
    out = []
    for q in range(PRIMS):
        a = q + 1 if q < BONES else q - BONES
        b = PARENT[a] if q < BONES else a
        rad = r if q < BONES else np.float64(1.5) * r
        with np.errstate(all='ignore'):
            abx, aby = u[b] - u[a], v[b] - v[a]
            out.append({'ax': u[a], 'ay': v[a], 'abx': abx, 'aby': aby, 'l2': abx * abx + aby * aby, 'r2': rad * rad,
                        'key': (z[a] + z[b]) * np.float64(0.5) if q < BONES else z[a], 'ok': bool(ok[a] and ok[b]), 'colour': a})
    return out, int((~ok).sum())


def skeleton_panel(joints, K, E, height, width, bone_px, palette, bgcolor_u8):
    """-> {'img' uint8 [H,W,3], 'dropped' joints dropped, 'covered' pixels covered, 'winner' int32 [H,W] the primitive a
    pixel shows (-1: background), 'n_cover' int32 [H,W] how many primitives cover its sample}.  Pixel (i, j) is sampled at
    (u, v) = (j, i).  Among the covering primitives the smallest key wins, at equal keys the higher index."""
    H, W = int(height), int(width)
    assert H >= 1 and W >= 1
    palette, bg = np.asarray(palette), np.asarray(bgcolor_u8)
    assert palette.shape == (JOINTS, 3) and palette.dtype == np.uint8 and bg.shape == (3,) and bg.dtype == np.uint8
    prims, dropped = primitives(joints, K, E, bone_px)
    px = np.arange(W, dtype=np.float64)[None, :] + np.zeros((H, 1))
    py = np.arange(H, dtype=np.float64)[:, None] + np.zeros((1, W))
    winner = np.full((H, W), -1, dtype=np.int32)
    best_key = np.zeros((H, W), dtype=np.float64)
    n_cover = np.zeros((H, W), dtype=np.int32)
    for q, p in enumerate(prims):
        if not p['ok']:
            continue
        with np.errstate(all='ignore'):
            dx, dy = px - p['ax'], py - p['ay']
            ex, ey = dx, dy
            if p['l2'] != 0.0:
                s = (dx * p['abx'] + dy * p['aby']) / p['l2']
                s = np.where(s < 0.0, 0.0, np.where(s > 1.0, 1.0, s))
                ex = px - (p['ax'] + s * p['abx'])
                ey = py - (p['ay'] + s * p['aby'])
            d2 = ex * ex + ey * ey
            cover = d2 <= p['r2']
        take = cover & ((winner < 0) | (p['key'] <= best_key))
        winner[take] = q
        best_key[take] = p['key']
        n_cover += cover
    img = np.empty((H, W, 3), dtype=np.uint8)
    img[:] = bg
    hit = winner >= 0
    colour = np.array([p['colour'] for p in prims], dtype=np.int64)
    img[hit] = palette[colour[winner[hit]]]
    return {'img': img, 'dropped': dropped, 'covered': int(hit.sum()), 'winner': winner, 'n_cover': n_cover}
