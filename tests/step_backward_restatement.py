"""Float64 restatements of the training step's two scatter / scan backward kernels (occnerf_amd/csrc/train_ops.hip), the truth
tests/test_e_step_backward.py holds them to PER ENTRY, and tests/test_step_backward_restatement.py keeps honest on the CPU.

warp_backward_kernel: d(mask)/d(vol, Rs, Ts)
--------------------------------------------
The library is built with -ffp-contract=off, so every fp32 product of the kernel is rounded on its own and `warp_backward_numpy`
forms every term with the kernel's roundings (fl = round to fp32):

    p      = fl(o + fl(d z))                                              per ray sample, z the sampler's own fp32 value
    pos_c  = fl(fma(R[c,2], p2, fma(R[c,1], p1, fl(R[c,0] p0))) + T_c)     the one fused chain: fma32
    gi_c   = fl(fl(fl(fl(fl(fl(pos_c - bmin_c) bscale_c) - 1) + 1) / 2) 31)  (the division by two is exact: five roundings)
    f      = floor(gi); the sample counts for this bone when -1 <= f <= 32 on all three axes and g != 0
    w_x    = {fl((x0 + 1) - gi_x), fl(gi_x - f_x)}, the same for y and z
    tap    = fl(g fl(fl(w_x w_y) w_z))       added to voxel (z0 + cz, y0 + cy, x0 + cx) when that lies inside the 32^3 volume
    dix    = sum over the in-bounds taps, in the order cz, cy, cx, each step rounded, of fl(fl(+-v w_y) w_z); diy, diz alike
    dp_c   = fl(fl(fl(g di_c) bscale_c) 15.5)
    d Rs[c,k] term = fl(dp_c p_k),   d Ts[c] term = dp_c

A kernel and this file then differ ONLY in the order and precision of the sums, and the bounds below are worst cases of those
sums, counted, not measured (u = 2^-24, gamma_k = k u / (1 - k u); W slices, `per` samples per slice; per entry A = the
float64 sum of |terms| and n their number):

  volume   gamma_W A + n 2^-53 A.  A workgroup adds its slice's terms into an fp64 LDS cell (each fp32 term is exact there;
           n_slice - 1 additions of relative error 2^-53), rounds the cell to fp32 once, and torch sums the W partials in fp32
           in some order (at most W - 1 additions per partial): at most W fp32 roundings touch a term.  A voxel with one term
           is bit-equal to it (every other partial is an exact zero), a voxel without terms is exactly zero, and so is every
           channel >= nb.
  Rs, Ts   gamma_{ceil(per / 256) + 6 + 1 + W} A.  A thread adds its <= ceil(per / 256) samples serially in fp32; 6 xor-shuffle
           levels add the 64 lanes; the wave total is widened to fp64, the four waves are added there (3 additions of 2^-53)
           and the sum is rounded to fp32 once; torch adds the W partials.  The thread's first addition (0 + t) and one of the
           W partial additions are exact, so the count is two roundings above what a term can meet; that slack also holds the
           three fp64 additions.

`warp_backward_numpy(..., exact=True)` evaluates the same formulas on the same fp32 inputs WITHOUT any rounding (float64
throughout): what torch's float64 autograd computes.  Where the grid coordinates are exact in both formats (the `dyadic`
case) the two modes scatter to the same voxels and differ by the three fp32 roundings of a tap, gamma_3 A.

composite_backward_kernel: d(rgb, acc, depth)/d(raw, mask)
----------------------------------------------------------
The kernel's expf / log1pf cannot be restated bit for bit, so the truth is torch's float64 autograd of train_path.raw2outputs on
the upcast fp32 inputs, and every entry is tied to its own scale by a condition weight B, the same gradient formula evaluated
in float64 with every term replaced by its absolute value (so B >= |gradient| entry-wise):

    Gh_s = |g_r c0| + |g_g c1| + |g_b c2| + |g_d z| + |g_a| + sum_c |g_c bg_c| / 255
    D_s  = Gh_s |T_s| + (sum_{j > s} Gh_j |w_j|) / |tt_s|
    B(d_raw[s, 3]) = D_s |mask dist em softplus'(x)|      softplus' = sigmoid(x), 1 above the switch point x > 20
    B(d_mask[s])   = D_s |1 - em|
    B(d_raw[s, c]) = |g_c| |w_s| c (1 - c)                c = 0, 1, 2
    d_raw[s, 4] = 0, and an entry with B = 0 is exactly 0.

The issue's tolerance scale S u B was measured first, on the fp32 reference, and is wrong: on the random rows rho_ref = max
err_ref32 / (S u B) is 135 at S = 2, 540 at S = 64 and 18 000 at S = 256 (130 x, not flat; 8.4e6 on the x = -30 ray), because B
takes no absolute value inside `1 - em` and `1 - c`: where em is close to 1 the rounding of em alone (u em) is thousands of
times u |1 - em|, and that error of alpha then travels through T and the suffix sum to every other entry of the ray.  Under a
tolerance of 4 rho_ref S u B nearly every entry would be free to be wrong by its own size.  As the issue asks for that case,
the scale is replaced by what the data shows, a first-order running error weight E >= B (all in float64, units of u):

    |d em|    e_s  = em_s (1 + softplus(x_s) dist_s)            exp's ulp and the rounding of its argument
    |d alpha| a_s  = |alpha_s| + |mask_s| e_s
    |d tt|    t_s  = a_s + |tt_s|
    |d T|     |T_s| tau_s,  tau_s = sum_{j < s} (t_j / |tt_j| + 1)
    |d w|     om_s = a_s |T_s| + |alpha_s| |T_s| tau_s + |w_s|
    |d R|     dR_s = sum_{j > s} (Gh_j om_j + (S + 4) Gh_j |w_j|)   (the suffix sum's own <= S additions: the issue's S u B)
    |d dalpha|     = Gh_s |T_s| (3 + tau_s) + dR_s / |tt_s| + (sum_{j > s} Gh_j |w_j|) / |tt_s| (1 + t_s / |tt_s|)
    E(d_mask[s])   = |d dalpha| |1 - em| + D_s (|1 - em| + e_s)
    E(d_raw[s, 3]) = |d dalpha| |mask dist em softplus'| + D_s |mask dist softplus'| (e_s + 4 em)
    E(d_raw[s, c]) = |g_c| (om_s c (1 - c) + |w_s| c)

An entry passes when (err - floor) / (u E) <= 4 max(rho_ref, 1), where rho_ref is the same ratio of the SAME autograd run in
fp32 by torch on the CPU: the constant is measured against the reference, never against the kernel; 4 covers the device's
exp / log1p (a few ulp each) and another scan order.  rho_ref is taken per (S, background, kind of ray) and never below the
value of the random rows of the same launch.  With E it is flat: random rows 0.75, 1.26, 0.80, 0.90, 0.91, 0.97, 0.93, 0.79,
1.11 at S = 1, 2, 63, 64, 65, 128, 129, 192, 256, and below 1 on every special kind of ray
(tests/test_step_backward_restatement.py prints them).  B keeps its two exact duties: B >= |gradient|, and B = 0 means an
exact zero.  `floor` is the absolute term no relative bound can hold, an fp32 underflow (2^-126) of T, em or w (the ray of
direction norm 1e3 reaches all three): 2^-126 times the entry's formula with those factors at 1."""
import numpy as np
import torch

from tests.encoder_backward_restatement import U32, U64, gamma  # noqa: F401
from tests.test_encoder_restatement import F32, fma32

G = 32                                                   # the kernel's kVolG
ETA32 = 2.0 ** -126                                      # smallest normal fp32


def slices_and_per(total):
    """occnerf_warp_backward_slices and the launch's samples per slice, restated (train_ops.hip:395-419)."""
    W = min(max((total + 16383) // 16384, 1), 16)
    return W, (total + W - 1) // W


def warp_backward_numpy(rays8, z, g_mask, Rs, Ts, vol, bmin, bscale, exact=False):
    """-> dict: vol_ssum / vol_A [C, 32, 32, 32] float64 and vol_n int64 (C = vol's channels; channels >= nb hold no term),
    rt_ssum / rt_A [nb, 12] (9 of Rs row-major, 3 of Ts) and rt_n [nb], gi [nb, N, 3] and `counted` [nb, N].
    exact: no rounding anywhere (float64 on the same inputs); rt_A is then the sum over the taps' absolute values."""
    ft = np.float64 if exact else F32

    def fl(a):
        return np.asarray(a, ft)
    rays8, z, g = np.asarray(rays8, F32), np.asarray(z, F32), np.asarray(g_mask, F32).reshape(-1)
    Rs, Ts, vol = np.asarray(Rs, F32), np.asarray(Ts, F32), np.asarray(vol, F32)
    bmin, bscale = np.asarray(bmin, F32).astype(ft), np.asarray(bscale, F32).astype(ft)
    n, S = z.shape
    nb, C = Rs.shape[0], vol.shape[0]
    assert vol.shape[1:] == (G, G, G) and C >= nb and g.shape == (n * S,)
    o, d = rays8[:, None, 0:3].astype(ft), rays8[:, None, 3:6].astype(ft)
    p = fl(o + fl(d * z[..., None].astype(ft))).reshape(-1, 3)
    live = g != 0
    p, g = p[live], g[live].astype(ft)
    nvox = G * G * G
    out = {'vol_ssum': np.zeros((C, nvox)), 'vol_A': np.zeros((C, nvox)), 'vol_n': np.zeros((C, nvox), np.int64),
           'rt_ssum': np.zeros((nb, 12)), 'rt_A': np.zeros((nb, 12)), 'rt_n': np.zeros(nb, np.int64),
           'gi': np.zeros((nb, n * S, 3), ft), 'counted': np.zeros((nb, n * S), bool)}
    half = ft(15.5)
    for b in range(nb):
        R, T = Rs[b].astype(ft), Ts[b].astype(ft)
        gi = np.empty((len(p), 3), ft)
        for c in range(3):
            if exact:
                pos = R[c, 2] * p[:, 2] + (R[c, 1] * p[:, 1] + R[c, 0] * p[:, 0]) + T[c]
            else:
                pos = fl(fma32(R[c, 2], p[:, 2], fma32(R[c, 1], p[:, 1], fl(R[c, 0] * p[:, 0]))) + T[c])
            gc = fl(fl(fl(pos - bmin[c]) * bscale[c]) - ft(1))
            gi[:, c] = fl(fl(fl(gc + ft(1)) / ft(2)) * ft(G - 1))
        f = np.floor(gi)
        with np.errstate(invalid='ignore'):
            ok = ((f >= -1) & (f <= G)).all(1)
        out['gi'][b, live] = gi
        out['counted'][b, live] = ok
        gi, f, pp, gg = gi[ok], f[ok], p[ok], g[ok]
        i0 = f.astype(np.int64)
        w = [(fl((i0[:, a] + 1).astype(ft) - gi[:, a]), fl(gi[:, a] - f[:, a])) for a in range(3)]     # [axis][corner]
        bv = vol[b].reshape(-1).astype(ft)
        di = [np.zeros(len(gi), ft) for _ in range(3)]
        di_abs = [np.zeros(len(gi)) for _ in range(3)]
        for cz in range(2):
            for cy in range(2):
                for cx in range(2):
                    xx, yy, zz = i0[:, 0] + cx, i0[:, 1] + cy, i0[:, 2] + cz
                    inb = (xx >= 0) & (xx < G) & (yy >= 0) & (yy < G) & (zz >= 0) & (zz < G)
                    vox = ((zz * G + yy) * G + xx)[inb]
                    wx, wy, wz = w[0][cx][inb], w[1][cy][inb], w[2][cz][inb]
                    t = fl(gg[inb] * fl(fl(wx * wy) * wz)).astype(np.float64)
                    out['vol_ssum'][b] += np.bincount(vox, weights=t, minlength=nvox)
                    out['vol_A'][b] += np.bincount(vox, weights=np.abs(t), minlength=nvox)
                    out['vol_n'][b] += np.bincount(vox, minlength=nvox)
                    v = bv[vox]
                    for a, (sign, wa, wb) in enumerate(((cx, wy, wz), (cy, wx, wz), (cz, wx, wy))):
                        step = fl(fl((v if sign else -v) * wa) * wb)
                        di[a][inb] = fl(di[a][inb] + step)
                        di_abs[a][inb] += np.abs(step)
        out['rt_n'][b] = len(gi)
        for c in range(3):
            dp = fl(fl(fl(gg * di[c]) * bscale[c]) * half)
            dp_abs = np.abs(gg) * di_abs[c] * float(bscale[c]) * 15.5
            for k in range(3):
                t = fl(dp * pp[:, k]).astype(np.float64)
                out['rt_ssum'][b, c * 3 + k] = t.sum()
                out['rt_A'][b, c * 3 + k] = (dp_abs * np.abs(pp[:, k])).sum() if exact else np.abs(t).sum()
            out['rt_ssum'][b, 9 + c] = dp.astype(np.float64).sum()
            out['rt_A'][b, 9 + c] = dp_abs.sum() if exact else np.abs(dp.astype(np.float64)).sum()
    for k in ('vol_ssum', 'vol_A', 'vol_n'):
        out[k] = out[k].reshape(C, G, G, G)
    return out


def bound_volume(A, n, W):
    return gamma(W) * A + n * U64 * A


def bound_rt(A, W, per):
    return gamma(-(-per // 256) + 6 + 1 + W) * A


def check(name, got, ssum, bound, n, bit_equal_single=False, where=None):
    """|got - ssum| <= bound per entry (an entry without terms, bound 0, must be exactly zero); entries of one term bit-equal to
    the fp32 term.  Prints and returns the worst error / bound; raises naming the worst entry (`where`: index -> text)."""
    got64 = np.asarray(got, np.float64)
    assert got64.shape == ssum.shape == bound.shape, (name, got64.shape, ssum.shape, bound.shape)
    assert np.isfinite(got64).all(), f'{name}: {int((~np.isfinite(got64)).sum())} entries are not finite'
    err = np.abs(got64 - ssum)
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    worst = float(ratio.max()) if ratio.size else 0.0
    n = np.broadcast_to(np.asarray(n), got64.shape)
    print(f'   {name}: worst error / bound {worst:.3f} over {int((bound > 0).sum())} entries with terms of {bound.size} '
          f'(fullest {int(np.max(n)) if n.size else 0} terms)')
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, np.where(bound > 0, ratio, np.inf), -1.0)), err.shape)
        raise AssertionError(f'{name}: {int(bad.sum())} entries over their bound; worst at {where(i) if where else i}: '
                             f'got {float(got64[i])!r}, float64 sum {float(ssum[i])!r}, bound {bound[i]:.3e}')
    if bit_equal_single:
        one = n == 1
        want = (ssum[one] + 0.0).astype(F32)                   # (0 + -0 = +0: what a zeroed tile holds)
        same = np.asarray(got)[one].astype(F32).view(np.uint32) == want.view(np.uint32)
        assert same.all(), f'{name}: {int((~same).sum())} single-term entries are not bit-equal to their fp32 term'
    return worst


def voxel_name(W, per, S):
    def where(i):
        b, zz, yy, xx = (int(v) for v in i)
        return f'bone {b} voxel (z {zz}, y {yy}, x {xx}), half {zz // 16}; {W} slices of {per} samples, S = {S}'
    return where


def rt_name(i):
    b, e = int(i[0]), int(i[1])
    return f'bone {b} ' + (f'Rs[{e // 3}, {e % 3}]' if e < 9 else f'Ts[{e - 9}]')


def check_warp(name, d_vol, d_Rs, d_Ts, ref, n_samples, S):
    """A device (or any fp32) result against `warp_backward_numpy`'s with the launch's own W and per."""
    W, per = slices_and_per(n_samples)
    nb = ref['rt_ssum'].shape[0]
    wv = check(f'{name} volume', d_vol, ref['vol_ssum'], bound_volume(ref['vol_A'], ref['vol_n'], W), ref['vol_n'],
               bit_equal_single=True, where=voxel_name(W, per, S))
    got_rt = np.concatenate([np.asarray(d_Rs).reshape(nb, 9), np.asarray(d_Ts).reshape(nb, 3)], 1)
    wr = check(f'{name} Rs/Ts', got_rt, ref['rt_ssum'], bound_rt(ref['rt_A'], W, per), ref['rt_n'][:, None], where=rt_name)
    return wv, wr


# ---- compositing ------------------------------------------------------------------------------------------------------
def _autograd(c, dtype):
    from occnerf_amd.train_path import raw2outputs

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    raw, mask = t(c['raw']).requires_grad_(True), t(c['mask']).requires_grad_(True)
    rgb, acc, depth, _ = raw2outputs(raw, mask[..., None], t(c['z']), t(c['rays8'][:, 3:6]), t(c['bg']))
    ((rgb * t(c['g_rgb'])).sum() + (acc * t(c['g_acc'])).sum() + (depth * t(c['g_depth'])).sum()).backward()
    return raw.grad.double().numpy(), mask.grad.double().numpy()


def composite_running_weights(c):
    """The float64 forward of a case and its first-order running error weights, in units of u (module docstring): dict of
    [n, S] arrays dist, sp, dsp, em, alpha, tt, T, w, e_s, a_s, t_s, tau_s, om_s, and col [n, S, 3].  The forward compositor's
    per-entry check (tests/composite_forward_restatement.py) builds its weights from the same a_s, t_s, tau_s, om_s."""
    raw, mask, z = (np.asarray(c[k], np.float64) for k in ('raw', 'mask', 'z'))
    n, S = z.shape
    dn = np.linalg.norm(np.asarray(c['rays8'], np.float64)[:, 3:6], axis=1)
    dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full((n, 1), 1e10)], 1) * dn[:, None]
    x = raw[..., 3]
    with np.errstate(over='ignore', under='ignore'):
        sp = np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))
        dsp = np.where(x > 20.0, 1.0, 1.0 / (1.0 + np.exp(-x)))
        em = np.exp(-sp * dist)
        col = 1.0 / (1.0 + np.exp(-raw[..., :3]))
    alpha = (1.0 - em) * mask
    tt = 1.0 - alpha + 1e-10
    T = np.concatenate([np.ones((n, 1)), np.cumprod(tt, 1)[:, :-1]], 1)
    w = alpha * T
    aT, att = np.abs(T), np.abs(tt)
    e = em * (1.0 + sp * dist)                                                  # |d em|: exp's own ulp and its argument's
    a = np.abs(alpha) + np.abs(mask) * e                                        # |d alpha|
    t = a + att                                                                 # |d tt|
    step = t / att + 1.0
    tau = np.concatenate([np.zeros((n, 1)), np.cumsum(step, 1)[:, :-1]], 1)     # |d T| / |T|
    omega = a * aT + np.abs(alpha) * aT * tau + np.abs(w)                       # |d w|
    return {'dist': dist, 'sp': sp, 'dsp': dsp, 'em': em, 'col': col, 'alpha': alpha, 'tt': tt, 'T': T, 'w': w, 'e_s': e, 'a_s': a,
            't_s': t, 'tau_s': tau, 'om_s': omega}


def composite_backward_float64(c):
    """c: a case of tests/step_backward_cases.py (fp32 arrays raw [n,S,5], mask, z [n,S], rays8, bg [3], g_rgb, g_acc, g_depth)
    -> dict d_raw [n,S,5], d_mask [n,S] (float64 autograd), B_raw, B_mask (condition weights), E_raw, E_mask (error weights), floor_raw, floor_mask (absolute terms)."""
    d_raw, d_mask = _autograd(c, torch.float64)
    mask, z = (np.asarray(c[k], np.float64) for k in ('mask', 'z'))
    g_rgb, g_acc, g_dep = (np.asarray(c[k], np.float64) for k in ('g_rgb', 'g_acc', 'g_depth'))
    bg = np.asarray(c['bg'], np.float64)
    n, S = z.shape
    rw = composite_running_weights(c)
    dist, sp, dsp, em, col, alpha, tt, T, w = (rw[k] for k in ('dist', 'sp', 'dsp', 'em', 'col', 'alpha', 'tt', 'T', 'w'))
    e, a, t, tau, omega = (rw[k] for k in ('e_s', 'a_s', 't_s', 'tau_s', 'om_s'))
    Gh = (np.abs(g_rgb[:, None, :] * col).sum(-1) + np.abs(g_dep[:, None] * z) + np.abs(g_acc)[:, None]
          + (np.abs(g_rgb * bg[None, :]).sum(-1) / 255.0)[:, None])
    gw = Gh * np.abs(w)
    tail = np.flip(np.cumsum(np.flip(gw, 1), 1), 1) - gw                       # sum over j > s
    D = Gh * np.abs(T) + tail / np.abs(tt)
    B_raw = np.zeros((n, S, 5))
    B_raw[..., :3] = np.abs(g_rgb)[:, None, :] * np.abs(w)[..., None] * col * (1.0 - col)
    lin = np.abs(mask * dist * dsp)
    B_raw[..., 3] = D * lin * em
    # E: the first-order rounding-error weight (see the module docstring), in units of u
    aT, aw, att = np.abs(T), np.abs(w), np.abs(tt)
    go = Gh * omega + (S + 4.0) * gw
    dR = np.flip(np.cumsum(np.flip(go, 1), 1), 1) - go                          # |d R|: sum over j > s
    dda = Gh * aT * (3.0 + tau) + dR / att + tail / att * (1.0 + t / att)       # |d dalpha|
    E_raw = np.zeros((n, S, 5))
    E_raw[..., :3] = np.abs(g_rgb)[:, None, :] * (omega[..., None] * col * (1.0 - col) + aw[..., None] * col)
    E_raw[..., 3] = dda * lin * em + D * lin * (e + 4.0 * em)
    E_mask = dda * np.abs(1.0 - em) + D * (np.abs(1.0 - em) + e)
    # floor: the entry's formula with T, em and w at 1 -- what an fp32 underflow (2^-126) of one of them can move
    ga = Gh * np.abs(alpha)
    coef = Gh + (np.flip(np.cumsum(np.flip(ga, 1), 1), 1) - ga) / att
    floor_raw = np.zeros((n, S, 5))
    floor_raw[..., :3] = ETA32 * np.abs(g_rgb)[:, None, :] * (col * (1.0 - col)) * np.abs(alpha)[..., None]
    floor_raw[..., 3] = ETA32 * coef * lin
    floor_mask = ETA32 * coef * (np.abs(1.0 - em) + 1.0)
    return {'d_raw': d_raw, 'd_mask': d_mask, 'B_raw': B_raw, 'B_mask': D * np.abs(1.0 - em), 'E_raw': E_raw, 'E_mask': E_mask,
            'floor_raw': floor_raw, 'floor_mask': floor_mask}


def composite_backward_ref32(c):
    """The same autograd in fp32 by torch on the CPU -> (d_raw, d_mask) as float64 arrays."""
    return _autograd(c, torch.float32)


def composite_ratio(got_raw, got_mask, ref, S):
    """Per ray: max over its entries of (err - floor) / (u E); inf where an entry with B = 0 is not exactly 0 or a value is
    not finite."""
    got_raw, got_mask = np.asarray(got_raw, np.float64), np.asarray(got_mask, np.float64)

    def ratio(got, want, B, E, floor):
        err = np.maximum(np.abs(got - want) - floor, 0.0)
        r = np.divide(err, U32 * E, out=np.zeros_like(err), where=B > 0)
        r[(B == 0) & (got != 0)] = np.inf
        r[~np.isfinite(got)] = np.inf
        return r
    r_raw = ratio(got_raw, ref['d_raw'], ref['B_raw'], ref['E_raw'], ref['floor_raw'])
    r_mask = ratio(got_mask, ref['d_mask'], ref['B_mask'], ref['E_mask'], ref['floor_mask'])
    return np.maximum(r_raw.reshape(len(r_raw), -1).max(1), r_mask.max(1)), r_raw, r_mask


def check_composite(name, c, got_raw, got_mask, ref=None, ref32=None):
    """The kernel's (or any) result against the float64 truth with the tolerance measured on the fp32 CPU reference, per kind
    of ray.  Prints rho_ref and the result's ratio per kind; raises naming the worst entry.  -> {kind: (rho_ref, ratio)}."""
    ref = composite_backward_float64(c) if ref is None else ref
    ref32 = composite_backward_ref32(c) if ref32 is None else ref32
    n, S = c['z'].shape
    rho, _, _ = composite_ratio(ref32[0], ref32[1], ref, S)
    got, r_raw, r_mask = composite_ratio(got_raw, got_mask, ref, S)
    assert np.isfinite(rho).all(), f'{name}: the fp32 reference itself breaks an exact zero on rays {np.flatnonzero(~np.isfinite(rho))}'
    base = float(rho[c['groups']['random']].max())
    seen, failures = {}, []
    for kind, rows in c['groups'].items():
        rho_k, got_k = float(rho[rows].max()), float(got[rows].max())
        seen[kind] = (rho_k, got_k)
        if not got_k <= 4.0 * max(rho_k, base, 1.0):
            r = int(rows[np.argmax(got[rows])])
            s, e = np.unravel_index(np.argmax(np.concatenate([r_raw[r], r_mask[r][:, None]], 1)), (S, 6))
            failures.append(f'{kind}: ratio {got_k:.3g} > 4 max(rho_ref {rho_k:.3g}, random rows {base:.3g}, 1) at ray {r} '
                            f'sample {s} ' + (f'd_raw[{e}]' if e < 5 else 'd_mask'))
    print(f'   {name}: rho_ref / result per kind: ' + ', '.join(f'{k} {a:.2g}/{b:.2g}' for k, (a, b) in seen.items()))
    assert not failures, f'{name}: ' + '; '.join(failures)
    return seen
