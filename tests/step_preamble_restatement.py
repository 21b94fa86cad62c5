"""Float64 restatements of the kernels that run once per training step -- the pose chain forward and backward, the prior
softmax, pack_rays (occnerf_amd/csrc/preamble.hip), the ConvTranspose3d gathers and agg_weights (csrc/train_ops.hip), the
per-point SDF backward (csrc/features.hip) and fused Adam (csrc/optim.hip) -- the truth tests/test_q_step_preamble_per_entry.py
holds them to PER ENTRY, and tests/test_step_preamble_restatement.py keeps honest on the CPU.  u = 2^-24 throughout.

Three kinds of check
--------------------
bit-equal      the arithmetic has no transcendental and a fixed order (col2im: bias, then the taps kd, kh, kw ascending, one
               rounded addition each; im2col and pack_rays: copies; agg_weights' `var` and the argument of its expf), or the
               operands are dyadic (the pose chain on signed permutations): no tolerance.
counted bound  every operation is a correctly rounded IEEE one (the library is built with -ffp-contract=off and no fast-math):
               Adam and the fp64 per-point SDF backward.  The counts stand with the functions below.
measured c     |got - r| <= c u E.  E is a first-order RUNNING ERROR weight: the chain is evaluated once more with `RE` values,
               pairs (value, error weight in units of u), so E follows the formula chain term by term and carries the first-order
               terms of the forward's own error (the backward recomputes the forward in fp32, so its E takes the forward's weights
               along).  An operation's weight joins what its operands' errors contribute to first order (b e_a and a e_b for a
               product, e_a and e_b for a sum, cos(x) e for a sine, ...) and |result| for its own rounding.  An entry whose E is 0
               (every term an exact zero) must be exactly 0.  c = 4 max(rho_ref, 1), rho_ref = max err / (u E) of torch's fp32
               CPU evaluation of the same chain on the same cases: measured on the reference, never on the kernel.

How the contributions are joined was measured first, on the reference, and the plain sum of absolute values is wrong here.  With
e = |b| e_a + |a| e_b + |v| and (K + 2) (|W| |h| + |b|) per dot product, the weights of the five layers compound by |W| |h| / |W h|
(8 to 16) per layer and those of the 23-bone kinematic chain by the absolute row sums of a rotation (up to sqrt 3) per level:
E(Rs) was 5 for the unrefined root and 1e6 for a hand bone, rho_ref per ENTRY 0.15 at the root and 1e-6 to 1e-3 everywhere else
(1e-7 for dW[0]), so 4 max(rho_ref, 1) would have left nearly every entry free to be wrong by thousands of u.  Rotations do not
amplify errors and independent roundings do not add linearly, so the contributions are joined by the root of the sum of their
squares (`_rss`): e = sqrt((b e_a)^2 + (a e_b)^2 + v^2), and a dot product of K terms carries
sqrt(sum_k (W_k e_k)^2 + K sum_k (W_k h_k)^2 + b^2 + z^2) (a serial fp32 sum of K terms walks sqrt(K) ||terms||_2).  This is no
longer a worst-case bound; c, measured on the reference, is what makes it a tolerance.  With it rho_ref is flat over entries,
outputs and cases (below).

The pose chain (`pose_chain`)
-----------------------------
One function states the forward and the hand-derived backward of pose_motion_bases_kernel / _backward_kernel in the kernels'
own operation order, and runs in three arithmetics: float64 (cross-checked against torch's float64 autograd of
BodyPoseRefiner -> rodrigues -> dst_Rs[1:] @ R -> MotionBasisComputer of occnerf_amd/modules.py, which is the truth the checks
use), RE (the weights E), and np.float32 (an emulated kernel, which the CPU tests run with planted defects).  The backward:

    f = C Ginv (C = cnl_gtfms):    dAi = C3^T dRs,  dti = C3^T dTs
    Ginv = [A^-1, -A^-1 T]:        dAi -= dti (x) T,  dT = -Ai^T dti,  dA = -Ai^T dAi Ai^T
    G_i = G_p L_i (i = 23 .. 1):   dRl_i = Rg_p^T dRg_i,  dRg_p += dRg_i Rl_i^T + dTg_i (x) Tl_i,  dTg_p += dTg_i
    Rl_j = dst_R_j Rod(r_j):       dRod = dst_R_j^T dRl_j,  dr_j = J_Rod(r_j)^T dRod   (theta = sqrt(1e-5 + |r|^2))
    five layers, batch 1:          dW_l = dz_l (x) h_l,  db_l = dz_l,  dz_{l-1} = (W_l^T dz_l) . [h_l > 0]

so E(dW[j,k]) joins E(dz[j]) |h[k]|, |dz[j]| E(h[k]) and |dW[j,k]|; E(dz) joins W^T E(dz) and sqrt(n) times the terms of W^T dz,
through the masks; and E(drvec) comes from the five stages above.  The constant 1e-5 of theta is 1e-5 in float64 and fl(1e-5) in
the kernel: it enters with weight 1e-5.  Condition on the cases: every hidden pre-activation has
|z| >= 4 (K + 2) u (|W| |h| + |b|), so fp32 and float64 agree on every ReLU (`relu_margin`; seeds 0 .. 11 give 0.3 to 93 times
(K + 2) u A, the committed ones 20.8, 28.0 and 45.6).  On the dyadic refine = 0 case every operation of the chain is exact in
fp32 and float64 alike (`pose_exact_truth` asserts it); torch's LU-based inverse is off by 6e-17 on 17 of its entries there and
serves only as a cross-check.

rho_ref (torch fp32 on the CPU; tests/test_step_preamble_restatement.py prints them and asserts the spread per check <= 10 x;
the value depends on the host's BLAS and thread count: a second machine gave 0.90, 0.78, 0.75 and 1.75 for the first line):

    pose forward    refine = 0 random 0.96;  refine = 1: reference init 0.78, default init 0.75, zero rows 0.86
    pose backward   all ten outputs together: reference init 1.13, default init 0.42, zero rows 0.45
                    per output over four seeds of each regime: 0.17 to 1.13
    prior softmax   0.17 to 0.65 over the fifteen (C, V) with C > 1 (C = 1: exactly 1, rho_ref 0)
    agg_weights     atts 0.25 to 0.38 for K <= 10, 0.07 to 0.09 for K = 39, 40 (the cases with random rows, N >= 255)

So c is 4 nearly everywhere and 4.5 for the backward at the reference's initialisation.

prior_softmax
-------------
r = softmax_c(dec_c + log prior_c) in float64.  q_c = 1 + |dec_c| + |log prior_c| + |x_c - m| + C and
E_c = r_c (q_c + sum_k r_k q_k): the entry's own exponent and quotient, and the denominator.  A channel whose prior is 0 gives
exactly 0, C = 1 gives exactly 1.  One absolute term no relative bound can hold: outputs below 2^-126 (dec = -30 and
prior = 1e-30 beside a channel at +30 reach e^-129) underflow in fp32, so the bound is c u E + 2^-126.

point_sdf_backward
------------------
The four lines above the kernel in float64 on the fp32 `dir` (`point_sdf_backward_f64`); `neg` comes from the fp32 rule of the
forward (oracle.point_sdf), a discrete value.  Bound u |r| + 64 2^-53 B: the store is the one fp32 rounding, B the
absolute-value evaluation.  The longest chain of fp64 operations a term passes is c_j (3 products, 2 additions, 1 division),
knn_base (product, 2 additions, division; 2 more additions for the denominator), nbr - knn_base, the 3-term dot product with
d_knn_base (product, 2 additions), / den, u = dir / |dir| with its 3 products, 2 additions and square root, c u, the difference,
the product with dc, / |dir|, gd u, their sum, and the 9 additions into g: 41 operations, rounded up to 64.  The kernel used to
take |dir| from the forward's fp32 norm3: off by up to u |dir|, which every term of g carries at full size while their sum
cancels -- an emulation of that missed the bound on a third of the rows, by up to 300 x.  It now forms |dir| in fp64.

Adam
----
`adam_ref`: adam1 in float64 on the fp32 operands and the fp32 constants the table holds; first-order counts per output
(d x = the bound of x; clip = 1 when the clip coefficient is not 1):

    g' = g coef                        d g' = clip u |g'|
    m' = m + (g' - m) (1 - beta1)      d m' = u (|m'| + |t| + (1 - beta1) |g' - m|) + (1 - beta1) d g'     t = (g' - m)(1 - beta1)
    v' = v beta2 + ((1 - beta2) g') g' d v' = u (|v'| + |v beta2| + 2 cc) + 2 cc clip u + 2^-126           cc = (1 - beta2) g'^2
    s = sqrt(v'), q = s / bc2_sqrt, den = q + eps, r = m' / den, k = lr / bc1, p' = p - k r
    d s = u s + min(d v' / (2 s), sqrt(d v')),  d q = u q + d s / bc2_sqrt,  d den = u den + d q,
    d r = u |r| + d m' / den + |r| d den / den,  d p' = u |p'| + u |k r| + |k| d r + u |k r|

each times (1 + 2^-20) for the second-order terms.  grad_norm: a gradient entry's square passes 1 product, at most 256 serial
additions of its thread (CHUNK / 256; the 16-byte path: 3 + 64), 6 shuffle levels, 2 additions of the four waves, the fp32
store of the fp64 total: n = 266 on the square, halved by the root, plus the root's own rounding:
|got - norm| <= (gamma_266 / 2 + 2 u) norm."""
import numpy as np
import torch

F32 = np.float32
U32 = 2.0 ** -24
U64 = 2.0 ** -53
ETA32 = 2.0 ** -126
SLACK = 1.0 + 2.0 ** -20


def gamma(k, u=U32):
    return k * u / (1.0 - k * u)


def _parents():
    from occnerf_amd.modules import SMPL_PARENT
    return tuple(SMPL_PARENT)


def _rss(*terms):
    """Root of the sum of squares: how independent first-order errors combine."""
    return np.sqrt(sum(np.square(np.asarray(t, np.float64)) for t in terms))


# ---- running-error values -------------------------------------------------------------------------------------------------
class RE:
    """(value, first-order error weight in units of u), float64 arrays of one shape."""
    __array_priority__ = 1000

    def __init__(self, v, e=None):
        self.v = np.array(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.array(np.broadcast_to(e, self.v.shape), np.float64)

    @staticmethod
    def lift(x):
        return x if isinstance(x, RE) else RE(x)

    def __getitem__(self, i):
        return RE(self.v[i], self.e[i])

    def __neg__(self):
        return RE(-self.v, self.e)

    def __add__(self, o):
        o = RE.lift(o)
        v = self.v + o.v
        return RE(v, _rss(self.e, o.e, v))

    __radd__ = __add__

    def __sub__(self, o):
        o = RE.lift(o)
        v = self.v - o.v
        return RE(v, _rss(self.e, o.e, v))

    def __rsub__(self, o):
        return RE.lift(o) - self

    def __mul__(self, o):
        o = RE.lift(o)
        v = self.v * o.v
        return RE(v, _rss(self.e * o.v, self.v * o.e, v))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = RE.lift(o)
        v = self.v / o.v
        return RE(v, _rss(self.e / o.v, v * o.e / o.v, v))

    def __rtruediv__(self, o):
        return RE.lift(o) / self

    def swapaxes(self, a, b):
        return RE(self.v.swapaxes(a, b), self.e.swapaxes(a, b))

    def reshape(self, *s):
        return RE(self.v.reshape(*s), self.e.reshape(*s))


def _val(x):
    return x.v if isinstance(x, RE) else np.asarray(x, np.float64)


def _sqrt(x):
    if isinstance(x, RE):
        v = np.sqrt(x.v)
        return RE(v, _rss(x.e / (2.0 * v), v))
    return np.sqrt(x)


def _sin(x):
    if isinstance(x, RE):
        v = np.sin(x.v)
        return RE(v, _rss(np.cos(x.v) * x.e, v))
    return np.sin(x)


def _cos(x):
    if isinstance(x, RE):
        v = np.cos(x.v)
        return RE(v, _rss(np.sin(x.v) * x.e, v))
    return np.cos(x)


def _stack(items, axis):
    if any(isinstance(a, RE) for a in items):
        items = [RE.lift(a) for a in items]
        return RE(np.stack([a.v for a in items], axis), np.stack([a.e for a in items], axis))
    return np.stack(items, axis)


def _cat(items):
    if any(isinstance(a, RE) for a in items):
        items = [RE.lift(a) for a in items]
        return RE(np.concatenate([a.v for a in items], 0), np.concatenate([a.e for a in items], 0))
    return np.concatenate(items, 0)


def _T(a):
    return a.swapaxes(-1, -2)


def _mm(A, B):
    """[..., r, 3] @ [..., 3, c], the three products added left to right (the kernels' order)."""
    return A[..., :, 0:1] * B[..., 0:1, :] + A[..., :, 1:2] * B[..., 1:2, :] + A[..., :, 2:3] * B[..., 2:3, :]


def _mat33(e):
    return _stack([_stack(e[0:3], -1), _stack(e[3:6], -1), _stack(e[6:9], -1)], -2)


# ---- the pose chain in three arithmetics ----------------------------------------------------------------------------------
def _dense(W, b, h, mode, order):
    """-> pre-activation z [out] and, in RE mode, A = |W| |h| + |b|."""
    K = W.shape[1]
    if mode == 're':
        A = np.abs(W) @ np.abs(h.v) + np.abs(b)
        z = W @ h.v + b
        return RE(z, _rss(np.sqrt((W * W) @ (h.e * h.e)), np.sqrt(K * ((W * W) @ (h.v * h.v))), b, z)), A
    if mode == 'f64':
        return W @ h + b, None
    acc = np.zeros(W.shape[0], F32)
    for k in (range(K) if order == 0 else range(K - 1, -1, -1)):
        acc = acc + W[:, k] * h[k]
    return acc + b, None


def _dense_T(W, dz, mode, order):
    n = W.shape[0]
    if mode == 're':
        v = W.T @ dz.v
        return RE(v, _rss(np.sqrt((W * W).T @ (dz.e * dz.e)), np.sqrt(n * ((W * W).T @ (dz.v * dz.v))), v))
    if mode == 'f64':
        return W.T @ dz
    acc = np.zeros(W.shape[1], F32)
    for j in (range(n) if order == 0 else range(n - 1, -1, -1)):
        acc = acc + W[j, :] * dz[j]
    return acc


def _relu(z):
    if isinstance(z, RE):
        return RE(np.maximum(z.v, 0.0), np.where(z.v > 0, z.e, 0.0))
    return np.maximum(z, z.dtype.type(0))


def _mask(x, h):
    live = _val(h) > 0
    if isinstance(x, RE):
        return RE(np.where(live, x.v, 0.0), np.where(live, x.e, 0.0))
    return np.where(live, x, x.dtype.type(0))


DEFECTS = ('parent13', 'mask3from2', 'drop_dTg_Tl', 'dtheta_sign', 'dT_no_transpose')


def pose_chain(c, mode='f64', refine=True, dRs=None, dTs=None, defect=None, order=0):
    """c: a case of tests/step_preamble_cases.py (float64 arrays exact in fp32: W[5], b[5], posevec[69], dst_Rs[24,3,3],
    dst_Ts[24,3], cnl_gtfms[24,4,4]).  mode 'f64' | 're' | 'f32'.  -> dict Rs [24,3,3], Ts [24,3], `margin` (RE mode: the smallest
    |z| / ((K + 2) u A) over the hidden pre-activations) and, with cotangents dRs [24,3,3], dTs [24,3], dW[5], db[5]."""
    assert defect is None or (defect in DEFECTS and mode == 'f32')
    ft = F32 if mode == 'f32' else np.float64

    def a(x):
        x = np.asarray(x, np.float64).astype(ft)
        return RE(x) if mode == 're' else x
    parent = list(_parents())
    if defect == 'parent13':
        parent[13] = 12
    if refine:
        W, b = [np.asarray(w, np.float64).astype(ft) for w in c['W']], [np.asarray(x, np.float64).astype(ft) for x in c['b']]
    dst_Rs, Tl = a(c['dst_Rs']), a(np.asarray(c['dst_Ts'])[:, :, None])
    G3, Gt = a(np.asarray(c['cnl_gtfms'])[:, :3, :3]), a(np.asarray(c['cnl_gtfms'])[:, :3, 3:4])
    one, two = (F32(1.0), F32(2.0)) if mode == 'f32' else (1.0, 2.0)
    out = {'margin': np.inf}
    Rl = dst_Rs
    if refine:
        h = [a(c['posevec'])]
        for l in range(5):
            z, A = _dense(W[l], b[l], h[l], mode, order)
            if l < 4:
                if mode == 're':
                    out['margin'] = min(out['margin'], float(np.min(np.abs(z.v) / ((W[l].shape[1] + 2) * U32 * A))))
                h.append(_relu(z))
        rvec = z.reshape(23, 3)
        rx, ry, rz = rvec[:, 0], rvec[:, 1], rvec[:, 2]
        eps = RE(np.full(23, 1e-5), 1e-5) if mode == 're' else np.full(23, 1e-5, ft)
        theta = _sqrt(eps + (rx * rx + ry * ry + rz * rz))
        x, y, zz = rx / theta, ry / theta, rz / theta
        cs, sn = _cos(theta), _sin(theta)
        oc = one - cs
        C = _mat33([x * x + (one - x * x) * cs, x * y * oc - zz * sn, x * zz * oc + y * sn,
                    x * y * oc + zz * sn, y * y + (one - y * y) * cs, y * zz * oc - x * sn,
                    x * zz * oc - y * sn, y * zz * oc + x * sn, zz * zz + (one - zz * zz) * cs])
        Rl = _cat([dst_Rs[0:1], _mm(dst_Rs[1:], C)])
    Rg, Tg = [Rl[0:1]], [Tl[0:1]]
    for i in range(1, 24):
        p = parent[i]
        Rg.append(_mm(Rg[p], Rl[i:i + 1]))
        Tg.append(_mm(Rg[p], Tl[i:i + 1]) + Tg[p])
    Rg, Tg = _cat(Rg), _cat(Tg)
    m = [[Rg[:, i, j] for j in range(3)] for i in range(3)]
    c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1]
    c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2]
    c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0]
    inv_det = one / (m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02)
    Ai = _mat33([c00 * inv_det, (m[0][2] * m[2][1] - m[0][1] * m[2][2]) * inv_det, (m[0][1] * m[1][2] - m[0][2] * m[1][1]) * inv_det,
                 c01 * inv_det, (m[0][0] * m[2][2] - m[0][2] * m[2][0]) * inv_det, (m[0][2] * m[1][0] - m[0][0] * m[1][2]) * inv_det,
                 c02 * inv_det, (m[0][1] * m[2][0] - m[0][0] * m[2][1]) * inv_det, (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * inv_det])
    ti = -_mm(Ai, Tg)
    Rs, Ts = _mm(G3, Ai), _mm(G3, ti) + Gt
    out['Rs'], out['Ts'] = Rs, Ts[:, :, 0]
    if dRs is None:
        return out
    assert refine
    dRs, dTs = a(dRs), a(np.asarray(dTs)[:, :, None])
    dAi, dti = _mm(_T(G3), dRs), _mm(_T(G3), dTs)
    dAi = dAi - dti * _T(Tg)
    dTg = -_mm(Ai if defect == 'dT_no_transpose' else _T(Ai), dti)
    dRg = -_mm(_mm(_T(Ai), dAi), _T(Ai))
    dRg, dTg = [dRg[i:i + 1] for i in range(24)], [dTg[i:i + 1] for i in range(24)]
    dRl = [None] * 24
    for i in range(23, 0, -1):
        p = parent[i]
        dRl[i] = _mm(_T(Rg[p:p + 1]), dRg[i])
        back = _mm(dRg[i], _T(Rl[i:i + 1]))
        if defect != 'drop_dTg_Tl':
            back = back + dTg[i] * _T(Tl[i:i + 1])
        dRg[p] = dRg[p] + back
        dTg[p] = dTg[p] + dTg[i]
    g = _mm(_T(dst_Rs[1:]), _cat(dRl[1:]))
    g = [g[:, k // 3, k % 3] for k in range(9)]
    dx = g[0] * (two * x * oc) + (g[1] + g[3]) * (y * oc) + (g[2] + g[6]) * (zz * oc) + (g[7] - g[5]) * sn
    dy = g[4] * (two * y * oc) + (g[1] + g[3]) * (x * oc) + (g[5] + g[7]) * (zz * oc) + (g[2] - g[6]) * sn
    dz_ = g[8] * (two * zz * oc) + (g[2] + g[6]) * (x * oc) + (g[5] + g[7]) * (y * oc) + (g[3] - g[1]) * sn
    dc = g[0] * (one - x * x) + g[4] * (one - y * y) + g[8] * (one - zz * zz) - \
        ((g[1] + g[3]) * (x * y) + (g[2] + g[6]) * (x * zz) + (g[5] + g[7]) * (y * zz))
    ds = (g[3] - g[1]) * zz + (g[2] - g[6]) * y + (g[7] - g[5]) * x
    dtheta = (ds * cs - dc * sn) - (dx * rx + dy * ry + dz_ * rz) / (theta * theta)
    if defect == 'dtheta_sign':
        dtheta = -dtheta
    dz = _stack([dx / theta + dtheta * rx / theta, dy / theta + dtheta * ry / theta, dz_ / theta + dtheta * rz / theta], -1).reshape(69)
    out['dW'], out['db'] = [None] * 5, [None] * 5
    for l in range(4, -1, -1):
        out['dW'][l] = dz[:, None] * h[l][None, :]
        out['db'][l] = dz
        if l:
            dz = _mask(_dense_T(W[l], dz, mode, order), h[l - 1] if (defect == 'mask3from2' and l == 4) else h[l])
    return out


def relu_margin(c):
    """Smallest |z| / ((K + 2) u (|W| |h| + |b|)) over the hidden pre-activations of the float64 chain; a case needs >= 4."""
    return pose_chain(c, 're', True)['margin']


def _torch_chain(c, dtype, refine, dRs=None, dTs=None):
    from occnerf_amd.modules import BodyPoseRefiner, MotionBasisComputer

    def t(x):
        return torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(dtype)
    dec = BodyPoseRefiner().to(dtype)
    lin = [m for m in dec.block_mlps if isinstance(m, torch.nn.Linear)]
    if refine:
        with torch.no_grad():
            for m, W, b in zip(lin, c['W'], c['b']):
                m.weight.copy_(t(W))
                m.bias.copy_(t(b))
    dst_Rs = t(c['dst_Rs'])
    if refine:
        refined = dec(t(c['posevec'])[None])['Rs'][0]
        dst_Rs = torch.cat([dst_Rs[0:1], torch.matmul(dst_Rs[1:], refined)], 0)
    Rs, Ts = MotionBasisComputer()(dst_Rs[None], t(c['dst_Ts'])[None], t(c['cnl_gtfms'])[None])
    out = {'Rs': Rs[0].detach().double().numpy(), 'Ts': Ts[0].detach().double().numpy()}
    if dRs is not None:
        params = [m.weight for m in lin] + [m.bias for m in lin]
        gr = torch.autograd.grad((Rs[0] * t(dRs)).sum() + (Ts[0] * t(dTs)).sum(), params, allow_unused=True)
        gr = [torch.zeros_like(p) if x is None else x for p, x in zip(params, gr)]
        out['dW'], out['db'] = [x.double().numpy() for x in gr[:5]], [x.double().numpy() for x in gr[5:]]
    return out


def pose_truth(c, refine, dRs=None, dTs=None):
    """torch's float64 evaluation (and autograd) of the modules: the truth."""
    return _torch_chain(c, torch.float64, refine, dRs, dTs)


def pose_exact_truth(c):
    """The dyadic refine = 0 case: every operation of the restated chain is exact there, in fp32 and float64 alike, so its
    float64 evaluation IS the value (torch's LU-based inverse is not exact on it and serves only to 1e-12)."""
    f64, f32 = pose_chain(c, 'f64', False), pose_chain(c, 'f32', False)
    for k in ('Rs', 'Ts'):
        assert np.array_equal(f64[k], f32[k].astype(np.float64)) and np.array_equal(f64[k] * 64.0, np.round(f64[k] * 64.0)), k
    return {'Rs': f64['Rs'], 'Ts': f64['Ts']}


def pose_ref32(c, refine, dRs=None, dTs=None):
    """The same in fp32 by torch on the CPU: what rho_ref is measured on."""
    return _torch_chain(c, torch.float32, refine, dRs, dTs)


def pose_weights(c, refine, dRs=None, dTs=None):
    """E per output, units of u."""
    r = pose_chain(c, 're', refine, dRs, dTs)
    out = {'Rs': r['Rs'].e, 'Ts': r['Ts'].e}
    if dRs is not None:
        out['dW'], out['db'] = [x.e for x in r['dW']], [x.e for x in r['db']]
    return out


def pose_outputs(res):
    """dict of a chain's outputs -> flat list of (name, array)."""
    items = [('Rs', res['Rs']), ('Ts', res['Ts'])]
    if 'dW' in res:
        items = [(f'dW[{l}]', res['dW'][l]) for l in range(5)] + [(f'db[{l}]', res['db'][l]) for l in range(5)]
    return items


# ---- the checks -----------------------------------------------------------------------------------------------------------
def ratio(got, want, E, floor=0.0):
    """Per entry (|got - want| - floor)+ / (u E); inf where E = 0 and got != 0, or got is not finite."""
    got, want, E = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(E, np.float64)
    assert got.shape == want.shape == E.shape, (got.shape, want.shape, E.shape)
    err = np.maximum(np.abs(got - want) - floor, 0.0)
    r = np.divide(err, U32 * E, out=np.zeros_like(err), where=E > 0)
    r[(E == 0) & (got != 0)] = np.inf
    r[~np.isfinite(got)] = np.inf
    return r


def check_bounded(name, got, want, E, c, floor=0.0):
    """|got - want| <= c u E + floor per entry, exact zeros where E = 0.  -> the worst ratio err / (u E)."""
    r = ratio(got, want, E, floor)
    worst = float(r.max()) if r.size else 0.0
    print(f'   {name}: worst error / (u E) {worst:.3g} (c = {c:.3g}) over {r.size} entries, {int((np.asarray(E) == 0).sum())} exact zeros')
    if not worst <= c:
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        raise AssertionError(f'{name}: {int((r > c).sum())} entries over c u E (c = {c:.3g}); worst ratio {worst:.3g} at {tuple(int(v) for v in i)}: '
                             f'got {float(np.asarray(got, np.float64)[i])!r}, float64 {float(np.asarray(want)[i])!r}, '
                             f'u E {U32 * float(np.asarray(E)[i]):.3e}')
    return worst


def check_equal(name, got, want):
    """Every entry equal to `want` as a number of its own format (a signed zero equals a zero); `want` float64 must be exact in fp32
    where `got` is fp32."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if got.dtype == F32:
        assert np.array_equal(want.astype(F32).astype(np.float64), want.astype(np.float64)), f'{name}: the expected values are not exact in fp32'
    bad = ~(got.astype(np.float64) == want.astype(np.float64))
    if bad.any():
        i = np.unravel_index(int(np.argmax(bad)), bad.shape)
        raise AssertionError(f'{name}: {int(bad.sum())} of {bad.size} entries are not bit-equal; first at {tuple(int(v) for v in i)}: '
                             f'got {float(got[i])!r}, expected {float(want[i])!r}')


def check_abs(name, got, want, bound):
    """|got - want| <= bound per entry (a counted bound).  -> worst error / bound."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    assert got.shape == want.shape == bound.shape, (name, got.shape, want.shape, bound.shape)
    assert np.isfinite(got).all(), f'{name}: {int((~np.isfinite(got)).sum())} entries are not finite'
    err = np.abs(got - want)
    r = np.divide(err, bound, out=np.where(err > 0, np.inf, 0.0), where=bound > 0)
    worst = float(r.max()) if r.size else 0.0
    print(f'   {name}: worst error / bound {worst:.3g} over {r.size} entries')
    if not worst <= 1.0:
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        raise AssertionError(f'{name}: {int((r > 1).sum())} entries over their bound; worst {worst:.3g} at {tuple(int(v) for v in i)}: '
                             f'got {float(got[i])!r}, float64 {float(want[i])!r}, bound {float(bound[i]):.3e}')
    return worst


def c_of(rho_ref):
    return 4.0 * max(float(rho_ref), 1.0)


def check_pose(name, got, truth, E, ref32):
    """got / truth / E / ref32: dicts of one chain evaluation (pose_outputs).  c from the reference's worst ratio over all the
    outputs of the case.  -> (rho_ref, worst ratio of `got`)."""
    rho = max(float(ratio(b, t, e).max()) for (_, b), (_, t), (_, e) in zip(pose_outputs(ref32), pose_outputs(truth), pose_outputs(E)))
    assert np.isfinite(rho), f'{name}: the fp32 reference itself breaks an exact zero'
    worst = 0.0
    for (k, g), (_, t), (_, e) in zip(pose_outputs(got), pose_outputs(truth), pose_outputs(E)):
        worst = max(worst, check_bounded(f'{name} {k}', np.asarray(g, np.float64).reshape(np.shape(t)), t, e, c_of(rho)))
    return rho, worst


def path_to_root(b):
    parent, out = _parents(), set()
    while b > 0:
        out.add(b)
        b = parent[b]
    return out


# ---- prior softmax --------------------------------------------------------------------------------------------------------
def prior_softmax_ref(dec, prior):
    """dec, prior [C, V] -> r, E (units of u)."""
    dec, prior = np.asarray(dec, np.float64), np.asarray(prior, np.float64)
    C = dec.shape[0]
    with np.errstate(divide='ignore'):
        lp = np.log(prior)
    x = dec + lp
    m = x.max(0, keepdims=True)
    assert np.isfinite(m).all(), 'every voxel needs a positive prior'
    p = np.exp(x - m)
    r = p / p.sum(0, keepdims=True)
    live = prior > 0
    q = np.where(live, 1.0 + np.abs(dec) + np.abs(np.where(live, lp, 0.0)) + np.abs(np.where(live, x - m, 0.0)) + C, 0.0)
    return r, r * (q + (r * q).sum(0, keepdims=True))


def prior_softmax_ref32(dec, prior):
    t = torch.from_numpy(np.asarray(dec, F32)), torch.from_numpy(np.asarray(prior, F32))
    return torch.softmax(t[0] + torch.log(t[1]), 0).double().numpy()


def check_prior_softmax(name, got, dec, prior, rho_ref=None):
    r, E = prior_softmax_ref(dec, prior)
    rho = float(ratio(prior_softmax_ref32(dec, prior), r, E, ETA32).max()) if rho_ref is None else rho_ref
    got = np.asarray(got, np.float64)
    assert not got[np.asarray(prior) == 0].any(), f'{name}: a channel whose prior is 0 must be exactly 0'
    if r.shape[0] == 1:
        assert np.all(got == 1.0), f'{name}: with one channel every output is exactly 1'
    return rho, check_bounded(name, got, r, E, c_of(rho), ETA32)


# ---- ConvTranspose3d gathers ----------------------------------------------------------------------------------------------
def col2im(cols, bias, Cout, D, H, W, dtype=F32, defect=None):
    """cols [Cout * 64, D H W] -> out [Cout, 2D, 2H, 2W]: the bias first, then the taps in the order kd, kh, kw ascending, one
    addition of `dtype` each."""
    V = D * H * W
    cols = np.asarray(cols, np.float64).astype(dtype).reshape(Cout, 64, V)
    out = np.zeros((Cout, 2 * D, 2 * H, 2 * W), dtype)
    if bias is not None:
        out = out + np.asarray(bias, np.float64).astype(dtype)[:, None, None, None]

    def axis(n_out, n_in, t, kind):
        o = np.arange(n_out)
        k = ((o & 1) if (defect == 'kd_parity' and kind == 'd') else ((o + 1) & 1)) + 2 * t
        i = (o + 1 - k) >> 1
        return k, i, (i >= 0) & (i < n_in)
    co = np.arange(Cout)[:, None, None, None]
    for a in range(2):
        kd, id_, vd = axis(2 * D, D, a, 'd')
        for b in range(2):
            kh, ih, vh = axis(2 * H, H, b, 'h')
            for c in range(2):
                kw, iw, vw = axis(2 * W, W, c, 'w')
                k = kd[:, None, None] * 16 + kh[None, :, None] * 4 + kw[None, None, :]
                ok = vd[:, None, None] & vh[None, :, None] & vw[None, None, :]
                i3, h3, w3 = id_[:, None, None], ih[None, :, None], iw[None, None, :]
                v = (i3 * H + w3) * W + h3 if defect == 'swap_hw' else (i3 * H + h3) * W + w3
                tap = cols[co, k[None], np.where(ok, v, 0)[None] % V]
                out = np.where(ok[None], (out + tap).astype(dtype), out)
    return out


def im2col(gy, Cout, D, H, W):
    """gy [Cout, 2D, 2H, 2W] -> dcols [Cout * 64, D H W]: a copy, or an exact zero outside the output."""
    gy = np.asarray(gy).reshape(Cout, 2 * D, 2 * H, 2 * W)
    k = np.arange(64)[:, None, None, None]
    od = 2 * np.arange(D)[None, :, None, None] - 1 + (k >> 4)
    oh = 2 * np.arange(H)[None, None, :, None] - 1 + ((k >> 2) & 3)
    ow = 2 * np.arange(W)[None, None, None, :] - 1 + (k & 3)
    ok = (od >= 0) & (od < 2 * D) & (oh >= 0) & (oh < 2 * H) & (ow >= 0) & (ow < 2 * W)
    od, oh, ow = (np.broadcast_to(np.where(ok, x, 0), ok.shape) for x in (od, oh, ow))
    out = np.where(ok[None], gy[:, od, oh, ow], gy.dtype.type(0))
    return out.reshape(Cout * 64, D * H * W)


# ---- agg_weights ----------------------------------------------------------------------------------------------------------
def agg_weights_f32(counter, knn, defect=None):
    """The kernel's fp32 arithmetic in its order -> var [N] and the argument of expf [N, K], both fp32 and bit-exact."""
    a = np.asarray(counter, np.float64).astype(F32)[np.asarray(knn)]
    K = a.shape[1]
    amin = a.min(1)
    a = a + (F32(1.0) - amin)[:, None]
    a = a / a.max(1)[:, None]
    mean = np.zeros(len(a), F32)
    for j in range(K):
        mean = mean + a[:, j]
    mean = mean / F32(K)
    var = np.zeros(len(a), F32)
    for j in range(K):
        d = a[:, j] - mean
        var = var + d * d
    var = var / F32(K if defect == 'div_K' else K - 1)
    arg = a - a.max(1)[:, None]
    assert a.dtype == var.dtype == arg.dtype == F32
    return var, arg


def softmax_rows_ref(arg):
    """float64 softmax over the last axis of fp32 arguments (their max is 0) and E = r (K + 4)."""
    p = np.exp(np.asarray(arg, np.float64))
    r = p / p.sum(-1, keepdims=True)
    return r, r * (arg.shape[-1] + 4.0)


def softmax_rows_ref32(arg):
    return torch.softmax(torch.from_numpy(np.asarray(arg, F32)), -1).double().numpy()


def check_agg_weights(name, atts, var, counter, knn, rho_ref=None):
    """-> (rho_ref, worst ratio of atts)."""
    want_var, arg = agg_weights_f32(counter, knn)
    check_equal(f'{name} var', np.asarray(var, F32).reshape(-1), want_var)
    r, E = softmax_rows_ref(arg)
    rho = float(ratio(softmax_rows_ref32(arg), r, E).max()) if rho_ref is None else rho_ref
    atts = np.asarray(atts, F32)
    K = atts.shape[1]
    same = np.all(np.asarray(knn) == np.asarray(knn)[:, :1], 1)
    assert not want_var[same].any(), f'{name}: a row of equal ids has variance exactly 0'
    check_equal(f'{name} atts of the rows of equal ids', atts[same], np.full((int(same.sum()), K), F32(1.0) / F32(K), F32))
    return rho, check_bounded(f'{name} atts', atts, r, E, c_of(rho))


# ---- per-point SDF backward -----------------------------------------------------------------------------------------------
def knn3(pc, base):
    """Brute-force 3 nearest rows of `base` per row of `pc` (CPU stand-in for ops.knn_small)."""
    d = ((np.asarray(pc, np.float64)[:, None, :] - np.asarray(base, np.float64)[None]) ** 2).sum(-1)
    return np.argsort(d, 1, kind='stable')[:, :3].astype(np.int32)


def unit_normals(normals):
    n = np.asarray(normals, np.float64)
    return n / np.maximum(np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]), 1e-8)[:, None]


def sdf_dots32(pc, base, normals, kidx):
    """The forward's fp32 inside test (network.py:278): dot = fl(fl(fl(d0 n0) + fl(d1 n1)) + fl(d2 n2)) -> dot [P,3] fp32 and the
    float64 size |d0 n0| + |d1 n1| + |d2 n2| the cases' condition is stated on."""
    dir32 = np.asarray(pc, F32)[:, None, :] - np.asarray(base, F32)[kidx]
    n32 = np.asarray(normals, np.float64).astype(F32)[kidx]
    t = dir32 * n32
    return (t[..., 0] + t[..., 1]) + t[..., 2], np.abs(dir32.astype(np.float64) * n32.astype(np.float64)).sum(-1)


def point_sdf_backward_f64(pc, base, normals, unit, kidx, d_kb, d_dist, zero_dir_leak=False):
    """-> (d point_dist [P] float64, B [P]): the four lines above point_sdf_backward_kernel in float64 on the fp32 dir."""
    pc32, base32 = np.asarray(pc, F32), np.asarray(base, F32)
    kidx = np.asarray(kidx)
    dir_ = (pc32[:, None, :] - base32[kidx]).astype(np.float64)                  # [P, j, k], the fp32 difference
    nbr = base32[kidx].astype(np.float64)
    un = np.asarray(unit, np.float64)[kidx]
    nd = np.sqrt((dir_ ** 2).sum(-1))
    nd = np.where(nd < 1e-8, 1e-8, nd)
    u = dir_ / nd[..., None]
    cj = (dir_ * un).sum(-1) / nd
    att = np.abs(cj)
    den = att.sum(1)
    kb = (att[..., None] * nbr).sum(1) / den[:, None]
    dot32, _ = sdf_dots32(pc, base, normals, kidx)
    neg = (dot32 < 0).sum(1) > 1
    gd = np.asarray(d_dist, np.float64).reshape(-1) * np.where(neg, -1.0, 1.0) / 3.0
    d_kb = np.asarray(d_kb, np.float64)
    datt = (d_kb[:, None, :] * (nbr - kb[:, None, :])).sum(-1) / den[:, None]
    datt_abs = (np.abs(d_kb)[:, None, :] * (np.abs(nbr) + np.abs(kb)[:, None, :])).sum(-1) / den[:, None]
    sgn = np.sign(cj)
    if zero_dir_leak:
        sgn = np.where(cj == 0, 1.0, sgn)
    dc = sgn * datt
    g = (gd[:, None, None] * u + dc[..., None] * (un - cj[..., None] * u) / nd[..., None]).sum((1, 2))
    B = (np.abs(gd)[:, None, None] * np.abs(u)
         + (np.abs(sgn) * datt_abs)[..., None] * (np.abs(un) + np.abs(cj)[..., None] * np.abs(u)) / nd[..., None]).sum((1, 2))
    return g, B


def check_point_sdf_backward(name, got, g, B):
    return check_abs(name, np.asarray(got, np.float64).reshape(-1), g, U32 * np.abs(g) + 64.0 * U64 * B)


# ---- Adam -----------------------------------------------------------------------------------------------------------------
def adam_constants(lr, t, betas=(0.9, 0.999), eps=1e-8):
    """The fp32 constants of one step as occnerf_amd/optim.py and occnerf_adam_step form them."""
    import math
    b1, b2 = betas
    return {'lr': F32(lr), 'bc1': F32(1.0 - b1 ** t), 'bc2_sqrt': F32(math.sqrt(1.0 - b2 ** t)), 'beta2': F32(b2),
            'one_m_beta1': F32(1.0 - b1), 'one_m_beta2': F32(1.0 - b2), 'eps': F32(eps)}


def clip_coef32(norm_sq32, max_norm):
    """adam_kernel's clip coefficient from the device's fp32 squared norm, operation for operation (every one correctly rounded)."""
    if not max_norm or max_norm <= 0:
        return F32(1.0)
    c = F32(max_norm) / (np.sqrt(F32(norm_sq32)) + F32(1e-6))
    return c if c < F32(1.0) else F32(1.0)


def adam_ref(p, g, m, v, coef, k, swap_bc=False):
    """fp32 arrays and constants -> dict of (truth float64, bound) for 'exp_avg', 'exp_avg_sq', 'p' (the counts: module header)."""
    p, g, m, v = (np.asarray(x, F32).astype(np.float64) for x in (p, g, m, v))
    coef = float(F32(coef))
    clip = 0.0 if coef == 1.0 else 1.0
    c = {n: float(x) for n, x in k.items()}
    if swap_bc:
        c['bc1'], c['bc2_sqrt'] = c['bc2_sqrt'], c['bc1']
    u = U32
    g1 = g * coef
    d_g1 = clip * u * np.abs(g1)
    dgm = g1 - m
    t = dgm * c['one_m_beta1']
    m1 = m + t
    d_m1 = u * (np.abs(m1) + np.abs(t) + c['one_m_beta1'] * np.abs(dgm)) + c['one_m_beta1'] * d_g1
    a, cc = v * c['beta2'], c['one_m_beta2'] * g1 * g1
    v1 = a + cc
    d_v1 = u * (np.abs(v1) + np.abs(a) + 2.0 * cc) + 2.0 * cc * clip * u + np.where(cc > 0, ETA32, 0.0)
    s = np.sqrt(v1)
    d_s = u * s + np.minimum(np.divide(d_v1, 2.0 * s, out=np.full_like(s, np.inf), where=s > 0), np.sqrt(d_v1))
    q = s / c['bc2_sqrt']
    d_q = u * q + d_s / c['bc2_sqrt']
    den = q + c['eps']
    d_den = u * den + d_q
    r = m1 / den
    d_r = u * np.abs(r) + d_m1 / den + np.abs(r) * d_den / den
    kk = c['lr'] / c['bc1']
    st = kk * r
    p1 = p - st
    d_p1 = u * np.abs(p1) + 2.0 * u * np.abs(st) + abs(kk) * d_r
    return {'exp_avg': (m1, d_m1 * SLACK), 'exp_avg_sq': (v1, d_v1 * SLACK), 'p': (p1, d_p1 * SLACK)}


def adam1_f32(p, g, m, v, coef, k, swap_bc=False):
    """adam1 of csrc/optim.hip in np.float32, operation for operation (an emulated kernel for the CPU tests)."""
    p, g, m, v = (np.asarray(x, F32) for x in (p, g, m, v))
    bc1, bc2 = (k['bc2_sqrt'], k['bc1']) if swap_bc else (k['bc1'], k['bc2_sqrt'])
    g = g * F32(coef)
    m = m + (g - m) * k['one_m_beta1']
    v = v * k['beta2'] + k['one_m_beta2'] * g * g
    den = np.sqrt(v) / bc2 + k['eps']
    p = p - (k['lr'] / bc1) * (m / den)
    assert p.dtype == m.dtype == v.dtype == F32
    return p, m, v


def check_adam(name, p, m, v, ref):
    return {key: check_abs(f'{name} {key}', got, *ref[key]) for key, got in (('exp_avg', m), ('exp_avg_sq', v), ('p', p))}


def grad_norm_bound(norm64):
    return (gamma(266) / 2.0 + 2.0 * U32) * norm64


# ---- pack_rays ------------------------------------------------------------------------------------------------------------
def pack_rays_ref(rays, near, far, order=None):
    rays, near, far = np.asarray(rays, F32), np.asarray(near, F32).reshape(-1), np.asarray(far, F32).reshape(-1)
    src = np.arange(rays.shape[1]) if order is None else np.asarray(order)
    return np.concatenate([rays[0][src], rays[1][src], near[src, None], far[src, None]], 1)
