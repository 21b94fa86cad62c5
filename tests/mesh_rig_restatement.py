"""The numpy definition of the rig of the exported mesh: the skin weights read off the motion-weight
volume and the forward linear blend skinning they define.  csrc/mesh_rig.hip must give these bits.

Everything is float64 arithmetic on the float32 inputs with + - * / floor and comparisons only, one rounding per operator, in the
order written here (no fused multiply-add, no library sums): `a + b + c` below is always `(a + b) + c`.

  skin      c_b = canonical_weights() of tests/mesh_pose_restatement.py: every bone's trilinear tap at the canonical point;
            total = sum_b c_b in index order.  Selection, K times: among the bones not yet taken with c_b > 0 the largest c_b,
            on a tie the lower index.  n <= K bones are taken, s = their sum in selection order, w_k = float32(c_k / s);
            joints / weights in selection order, unused slots joint 0 and weight 0; count = n; kept = float32(s / total).
            n = 0: joint 0 with weight 1, kept 0.
  lbs       per frame and vertex, over the slots with w_k != 0 in slot order: q_k = R_b^T (x - T_b) in the order of the start
            point of pose_points; p = sum_k w_k q_k; posed = float32(p).  With targets: M = sum_k w_k R_b^T, r = target - p (the
            unrounded p), M d = r by _cramer; delta = float32(d), dflag 0; d = 0 and dflag 1 where det is 0 or not finite, the
            target's flag is not 0, or not every |d_c| <= max_delta."""
import numpy as np

from tests import mesh_pose_restatement as mp

_f64 = mp._f64


def skin(x_c, vol, bbox_min, bbox_scale, K=4):
    """-> (joints uint8 [n,K], weights float32 [n,K], count uint8 [n], kept float32 [n])."""
    K = int(K)
    if K not in (4, 8):
        raise ValueError(f'mesh_skin: K={K} is neither 4 nor 8')
    c = mp.canonical_weights(x_c, vol, bbox_min, bbox_scale)
    n, nb = c.shape
    total = np.zeros(n)
    for b in range(nb):
        total = total + c[:, b]
    taken = np.zeros((n, nb), dtype=bool)
    joints, cs, count = np.zeros((n, K), dtype=np.uint8), np.zeros((n, K)), np.zeros(n, dtype=np.uint8)
    rows = np.arange(n)
    for k in range(K):
        open_c = np.where(~taken & (c > 0.0), c, -np.inf)
        b = np.argmax(open_c, axis=1)                              # the first of equals: the lower index
        has = open_c[rows, b] > 0.0
        joints[has, k], cs[has, k] = b[has], c[rows, b][has]
        taken[rows[has], b[has]] = True
        count[has] += 1
    s = np.zeros(n)
    for k in range(K):
        s = s + cs[:, k]
    with np.errstate(all='ignore'):
        weights = np.where(cs > 0.0, cs / s[:, None], 0.0).astype(np.float32)
        kept = np.where(count > 0, s / total, 0.0).astype(np.float32)
    weights[count == 0, 0] = 1.0
    return joints, weights, count, kept


def lbs(x_c, joints, weights, Rs, Ts, target=None, target_flag=None, max_delta=0.05, parts=False):
    """Rs [F,nb,3,3], Ts [F,nb,3] -> posed float32 [F,V,3], with target [F,V,3] / target_flag [F,V] -> (posed, delta float32
    [F,V,3], dflag uint8 [F,V]).  parts=True: also the unrounded p [F,V,3] and M [F,V,3,3] (float64) behind them."""
    x, R, T = _f64(x_c).reshape(-1, 3), _f64(Rs), _f64(Ts)
    joints, w = np.asarray(joints, dtype=np.uint8), _f64(weights)
    F, nb = R.shape[0], R.shape[1]
    V, K = joints.shape
    p, M = np.zeros((F, V, 3)), np.zeros((F, V, 3, 3))
    for f in range(F):
        for k in range(K):
            use = (w[:, k] != 0.0) & (joints[:, k] < nb)
            b = np.where(use, joints[:, k], 0).astype(np.int64)
            d, Rb, wk = x - T[f, b], R[f, b], w[:, k]
            for j in range(3):
                q = (Rb[:, 0, j] * d[:, 0] + Rb[:, 1, j] * d[:, 1]) + Rb[:, 2, j] * d[:, 2]
                p[f, :, j] = np.where(use, p[f, :, j] + wk * q, p[f, :, j])
                for c in range(3):
                    M[f, :, j, c] = np.where(use, M[f, :, j, c] + wk * Rb[:, c, j], M[f, :, j, c])
    with np.errstate(over='ignore', invalid='ignore'):
        posed = p.astype(np.float32)
    if target is None:
        return (posed, p, M) if parts else posed
    t = _f64(target).reshape(F, V, 3)
    tf = np.asarray(target_flag, dtype=np.uint8).reshape(F, V)
    det, d = mp._cramer(M.reshape(-1, 3, 3), (t - p).reshape(-1, 3))
    with np.errstate(all='ignore'):
        ok = (det != 0.0) & np.isfinite(det) & (tf.reshape(-1) == 0) & np.all(np.abs(d) <= float(max_delta), axis=1)
        delta = np.where(ok[:, None], d, 0.0).astype(np.float32).reshape(F, V, 3)
    dflag = np.where(ok, 0, 1).astype(np.uint8).reshape(F, V)
    return (posed, delta, dflag, p, M) if parts else (posed, delta, dflag)


# ------------------------------------------------------------------ hand-made volumes of the tests
def ladder(nb, G=4, tie=None):
    """nb bones, constant channels 1, 2, .. nb (so every point inside the box has nb positive bones and the largest index
    wins); tie = (a, b): channel b takes channel a's value, so a and b tie everywhere.  (vol, bbox_min, bbox_scale)."""
    vol = np.stack([np.full((G, G, G), float(b + 1), np.float32) for b in range(nb)])
    if tie is not None:
        vol[tie[1]] = vol[tie[0]]
    return vol, np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)


def random_bases(F, nb, seed):
    """Rigid backward bases (Rs float32 [F,nb,3,3], Ts float32 [F,nb,3]): rotations by up to ~1 rad, offsets of decimetres."""
    from occnerf_amd import synth
    rng = np.random.RandomState(seed)
    Rs = np.stack([[synth.rodrigues_exact(rng.uniform(-0.6, 0.6, 3)) for _ in range(nb)] for _ in range(F)]).astype(np.float32)
    return Rs, rng.uniform(-0.2, 0.2, (F, nb, 3)).astype(np.float32)
