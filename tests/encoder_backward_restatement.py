"""Float64 restatement of the grid encoder's backward (gridencoder.cu:248-369), the truth the HIP backward kernels
(occnerf_amd/csrc/grid_encode.hip) and the C oracle's backward are tested against, with PER-CELL error budgets.

Every term of the scatter is formed exactly as the kernels form it -- cell position by one fp32 fma, fraction and corner
weight `(((1 * a0) * a1) * a2) * a3` with every product rounded to fp32, the term `fp32(w * g)` (float64 dispatch: the
double product `double(w) * g`, rounded once) -- so that a kernel and this file differ ONLY in the order of accumulation.
The sums are then taken in float64 (`np.bincount`), or in extended precision for the float64 dispatch.  Per table entry and
channel the restatement returns

    ssum   the float64 sum of the terms
    A      the float64 sum of their absolute values
    n      the number of terms (per entry: both channels get the same count)

and the tolerances below are worst-case bounds of the summation, not measurements (u = 2^-24, gamma_k = k u / (1 - k u),
Higham, Accuracy and Stability of Numerical Algorithms, section 4.2):

    serial fp32 sum (C oracle), fp32 atomics in any order (scatter kernel)    gamma_{n-1} A;   n = 1: bit-equal
    tiled kernel: fp64 LDS sums (n 2^-53 A), one rounding per slice to fp32,
      <= nsl fp32 atomic merges (nsl = 16 dense levels, 8 hashed)              gamma_{nsl+1} A + n 2^-53 A
    runs merged first (grid_grad_runs): a run of r <= 64 bitwise identical
      rows is summed in fp32 inside its 64-sample chunk before the product     + gamma_66 A
    float64 dispatch (double atomics in any order)                             n 2^-53 A

Rows outside [0, 1] contribute nothing."""
import numpy as np

from tests.test_encoder_restatement import F32, fma32, grid_index, level_scale

U32 = 2.0 ** -24
U64 = 2.0 ** -53


def gamma(k, u=U32):
    k = np.asarray(k, np.float64)
    return k * u / (1.0 - k * u)


def _level_corners(grad_l, xi, level, size, S, H, gridtype, align, interp, f64_terms):
    """One level: yields, per corner, (row int64 [n], terms float64 [n, C]) for the in-range inputs xi [n, D]."""
    D = xi.shape[1]
    scale = level_scale(level, S, H)
    res = int(np.ceil(scale)) + 1
    pos = fma32(xi, scale, F32(0.0 if align else 0.5))
    pg = np.floor(pos).astype(np.int64).astype(np.uint32)
    pos = (pos - pg.astype(F32)).astype(F32)
    if interp == 1:
        pos = (pos * pos * fma32(F32(-2.0), pos, F32(3.0))).astype(F32)
    for idx in range(1 << D):
        w = np.ones(len(xi), F32)
        pl = pg.copy()
        for d in range(D):
            if idx & (1 << d):
                w = (w * pos[:, d]).astype(F32)
                pl[:, d] = pg[:, d] + np.uint32(1)
            else:
                w = (w * (F32(1) - pos[:, d]).astype(F32)).astype(F32)
        row = grid_index(pl, size, res, gridtype, align).astype(np.int64)
        if f64_terms:
            t = w.astype(np.float64)[:, None] * grad_l                        # double(w) * g: one float64 rounding
        else:
            t = (w[:, None] * grad_l).astype(F32).astype(np.float64)           # fp32(w * g)
        yield row, t


def _prepare(grad, x, f64_terms):
    x = np.asarray(x, F32)
    grad = np.asarray(grad, np.float64 if f64_terms else F32)
    inr = ~((x < 0) | (x > 1)).any(1)
    return grad, x[inr], inr


def backward_numpy(grad, x, offsets, C, S, H, gridtype=0, align=False, interp=0):
    """grad [L, B, C] float32, x [B, D] -> (ssum [n_emb, C], A [n_emb, C], n [n_emb]); dense float64 arrays."""
    grad, xi, inr = _prepare(grad, x, False)
    L, n_emb = len(offsets) - 1, int(offsets[-1])
    ssum, sabs, cnt = np.zeros((n_emb, C)), np.zeros((n_emb, C)), np.zeros(n_emb, np.int64)
    for level in range(L):
        o0, size = int(offsets[level]), int(offsets[level + 1] - offsets[level])
        for row, t in _level_corners(grad[level][inr], xi, level, size, S, H, gridtype, align, interp, False):
            cnt[o0:o0 + size] += np.bincount(row, minlength=size)
            for c in range(C):
                ssum[o0:o0 + size, c] += np.bincount(row, weights=t[:, c], minlength=size)
                sabs[o0:o0 + size, c] += np.bincount(row, weights=np.abs(t[:, c]), minlength=size)
    return ssum, sabs, cnt


def backward_numpy_sparse(grad, x, offsets, C, S, H, gridtype=0, align=False, interp=0, f64_terms=False):
    """The same over the touched entries only -> (entry int64 [T] ascending, ssum [T, C], A [T, C], n [T]): no array of the
    table's size is made on the host.  f64_terms: the float64 dispatch's terms `double(w) * g`, summed in np.longdouble
    (64-bit significand on x86: the sum's own error is 2^-11 of the n 2^-53 A budget) and rounded once to float64."""
    grad, xi, inr = _prepare(grad, x, f64_terms)
    L = len(offsets) - 1
    acc = np.longdouble if f64_terms else np.float64
    out = []
    for level in range(L):
        o0, size = int(offsets[level]), int(offsets[level + 1] - offsets[level])
        rows, terms = zip(*_level_corners(grad[level][inr], xi, level, size, S, H, gridtype, align, interp, f64_terms)) \
            if len(xi) else ((), ())
        if not rows or not len(rows[0]):
            continue
        rows, terms = np.concatenate(rows), np.concatenate(terms)
        order = np.argsort(rows, kind='stable')
        rows, terms = rows[order], terms[order].astype(acc)
        starts = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]])
        out.append((rows[starts] + o0, np.add.reduceat(terms, starts, axis=0).astype(np.float64),
                    np.add.reduceat(np.abs(terms), starts, axis=0).astype(np.float64), np.diff(np.r_[starts, len(rows)])))
    if not out:
        return np.zeros(0, np.int64), np.zeros((0, C)), np.zeros((0, C)), np.zeros(0, np.int64)
    return tuple(np.concatenate(part) for part in zip(*out))


def input_grad_numpy(grad, dy_dx, D):
    """gridencoder.cu:343-369 in float64: gi[b, d] = sum_{l, c} grad[l, b, c] dy_dx[b, l, d, c] -> (gi, sum of |terms|)."""
    grad = np.asarray(grad, np.float64)
    L, B, C = grad.shape
    dy = np.asarray(dy_dx, np.float64).reshape(B, L, D, C)
    return np.einsum('lbc,bldc->bd', grad, dy), np.einsum('lbc,bldc->bd', np.abs(grad), np.abs(dy))


def input_grad_chain32(grad, dy_dx, D):
    """The fp32 kernel's fixed-order chain `r = r + g * dy` (multiply, round, add, round) over (level, channel)."""
    grad = np.asarray(grad, F32)
    L, B, C = grad.shape
    dy = np.asarray(dy_dx, F32).reshape(B, L, D, C)
    r = np.zeros((B, D), F32)
    for level in range(L):
        for c in range(C):
            r = (r + (grad[level, :, c, None] * dy[:, level, :, c]).astype(F32)).astype(F32)
    return r


# ---- per-cell budgets -------------------------------------------------------------------------------------------------
def bound_serial(A, n):
    """fp32 sum of n terms in any order (C oracle, scatter kernel)."""
    return gamma(np.maximum(np.asarray(n) - 1, 0))[:, None] * A


def bound_tiled(A, n, nsl):
    """tiled kernel; nsl: slices per tile of the entry's level (scalar or per entry)."""
    return (gamma(np.asarray(nsl, np.float64) + 1) * np.ones(len(A)))[:, None] * A + (np.asarray(n) * U64)[:, None] * A


def bound_runs(A):
    return gamma(66) * A


def bound_f64(A, n):
    return (np.asarray(n) * U64)[:, None] * A


def check(name, got, ssum, bound, n, bit_equal_single=True):
    """Assert |got - ssum| <= bound per cell (a cell without terms must be exactly zero) and, for cells with one term, bit
    equality with the fp32-rounded reference.  Prints and returns the worst error / bound ratio."""
    got64 = np.asarray(got, np.float64)
    err = np.abs(got64 - ssum)
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f'   {name}: worst error / bound {worst:.3f} over {int((np.asarray(n) > 0).sum())} touched cells '
          f'(fullest cell {int(np.max(n)) if len(n) else 0} terms)')
    bad = np.argwhere(err > bound)
    if len(bad):
        i, c = bad[np.argmax(ratio[bad[:, 0], bad[:, 1]])]
        raise AssertionError(f'{name}: {len(bad)} cells over their bound; worst at entry {i} channel {c}: got {got64[i, c]!r}, '
                             f'float64 sum {ssum[i, c]!r}, bound {bound[i, c]:.3e}, n = {int(n[i])}')
    if bit_equal_single:
        one = np.asarray(n) == 1
        want = (ssum[one] + 0.0).astype(F32)                       # (0 + -0 = +0: what a zero-initialised table holds)
        same = np.asarray(got)[one].astype(F32).view(np.uint32) == want.view(np.uint32)
        assert same.all(), f'{name}: {int((~same).sum())} single-term cells are not bit-equal to fp32(w * g)'
    return worst
