"""Float64 truth and per-entry check of composite_kernel (occnerf_amd/csrc/composite.hip), the forward of the renderer and of
the training step: tests/test_u_composite_forward_per_entry.py holds the kernel to it on the GPU,
tests/test_composite_forward_restatement.py keeps it honest on the CPU.

Truth: train_path.raw2outputs in float64 on the upcast fp32 inputs of a case of tests/step_backward_cases.py (rgb, acc, depth,
term; the per-sample weights, which raw2outputs does not return, by the same torch expressions).  The kernel's expf / log1pf
cannot be restated bit for bit, so this is the project's "measured c" check: every output entry is tied to a first-order
running error weight E, in units of u = 2^-24, built from the weights of the backward's restatement
(step_backward_restatement.composite_running_weights: a_s = |d alpha|, t_s = |d tt|, tau_s = |d T| / |T|, om_s = |d w|):

    E(w_s)   = om_s   (with one refinement: where alpha_j = 1 without any rounding -- em_j = 0 in float64, hence in fp32, and
                      mask_j = 1 -- tt_j is fl(1e-10) itself and sample j adds 2 to tau_s, not t_j / |tt_j| + 1 = 1e10; without it
                      a forward that omits the 1e-10 passes, every weight behind such a sample being free)
    E(acc)   = sum om_s + k_S sum |w_s|
    E(depth) = sum om_s |z_s| + k_S sum |w_s z_s|
    E(rgb_c) = sum (om_s c_s + 4 |w_s| c_s) + k_S sum |w_s c_s| + (E(acc) + 3 |1 - acc|) bg_c / 255

k_S = ceil(S / 64) + 6 is the number of additions a term can meet: a lane adds its ceil(S / 64) samples serially, then six
xor-shuffle levels add the 64 lanes.  4 |w_s| c_s: the sigmoid's exp, addition and division and the product w c; 3 |1 - acc|:
the subtraction, the product with bg and the division by 255.

An entry passes when (err - floor) / (u E) <= 4 max(rho_ref, 1).  rho_ref is the same ratio of torch's fp32 CPU evaluation of
the same function, per (S, background, kind of ray), never below the value of the random rows of the same launch: the constant
is measured against the reference, never against the kernel.  An entry with E = 0 (mask = 0: alpha, w exactly 0) must be
exactly right.  `floor` is what an fp32 underflow (2^-126) can move and no relative bound can hold: per sample
2^-126 (|alpha_s| (s + 1) + |mask_s| + 1) -- each of the <= s products that form T_s and T's product with alpha can lose
2^-126, later factors |tt| <= 1 do not grow it; em's underflow moves alpha by |mask| 2^-126; w's own -- and its sums for acc,
depth and rgb.

term (argmax alpha, first maximum): a_s is already the error weight of alpha.  Where the float64 maximum leads every other
sample of the ray by more than 4 max(rho_ref, 1) u (a_s + a_best), term must equal the float64 argmax; elsewhere it must name a
sample within that margin of the maximum.  Two rays are decided by construction: mask = 0 (every alpha is 0: sample 0) and,
where the saturated x = 25 ray holds samples with alpha = 1 exactly in float64, the first of them.

`forward_numpy32` is an fp32 numpy evaluation with a serial transmittance product; its `mutate` argument produces the wrong
answers the CPU test shows the check to refuse."""
import numpy as np
import torch

from tests.step_backward_restatement import ETA32, U32, composite_running_weights

F32 = np.float32
CHUNK = 64                                                # the kernel's wavefront: samples per scan chunk


def k_S(S):
    return -(-S // CHUNK) + 6


def forward_torch(c, dtype):
    """raw2outputs of the case in `dtype` by torch on the CPU -> dict of float64 arrays rgb [n,3], acc, depth [n], w, alpha [n,S]
    and term [n] (int64)."""
    import torch.nn.functional as Fn
    from occnerf_amd.train_path import raw2outputs

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    raw, mask, z, d, bg = t(c['raw']), t(c['mask']), t(c['z']), t(c['rays8'][:, 3:6]), t(c['bg'])
    rgb, acc, depth, term = raw2outputs(raw, mask[..., None], z, d, bg)
    # the per-sample weights, by raw2outputs' own lines (train_path.py:152-158)
    dists = torch.cat([z[..., 1:] - z[..., :-1], torch.full_like(z[..., :1], 1e10)], dim=-1) * torch.norm(d[..., None, :], dim=-1)
    alpha = (1.0 - torch.exp(-Fn.softplus(raw[..., 3]) * dists)) * mask
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1. - alpha + 1e-10], dim=-1), dim=-1)[:, :-1]
    w = alpha * trans
    assert torch.equal(w.sum(-1), acc), 'the restated weights are those raw2outputs summed'
    return {'rgb': rgb.double().numpy(), 'acc': acc.double().numpy(), 'depth': depth.double().numpy(), 'w': w.double().numpy(),
            'alpha': alpha.double().numpy(), 'term': term[:, 0].numpy().astype(np.int64)}


def composite_forward_float64(c):
    """-> dict: the float64 truth (rgb, acc, depth, w, alpha, term), the error weights E_* and floors floor_* of each output,
    and a_s [n,S]."""
    ref = forward_torch(c, torch.float64)
    rw = composite_running_weights(c)
    z, mask, bg = np.asarray(c['z'], np.float64), np.asarray(c['mask'], np.float64), np.asarray(c['bg'], np.float64)
    n, S = z.shape
    om, w, col, alpha = rw['om_s'], rw['w'], rw['col'], rw['alpha']
    # numpy's and torch's float64 terms are the same numbers up to their exp / log1p: a millionth of the unit u E they are held in
    assert np.all(np.abs(w - ref['w']) <= 1e-6 * U32 * om) and np.all(np.abs(alpha - ref['alpha']) <= 1e-6 * U32 * rw['a_s'])
    k = float(k_S(S))
    aw = np.abs(w)
    # alpha = 1 without any rounding (em = 0 in both formats, mask = 1): tt is fl(1e-10) itself, so the sample's step of tau_s is
    # 2 (tt's two roundings), not t_s / |tt_s| + 1 = 1e10, which would leave every later sample of the ray free to be anything
    exact = (rw['em'] == 0.0) & (mask == 1.0)
    less = np.where(exact, rw['t_s'] / np.abs(rw['tt']) + 1.0 - 2.0, 0.0)
    dtau = np.concatenate([np.zeros((n, 1)), np.cumsum(less, 1)[:, :-1]], 1)
    om = np.maximum(om - np.abs(alpha * rw['T']) * dtau, rw['a_s'] * np.abs(rw['T']) + aw)
    ref['E_w'] = om
    ref['E_acc'] = om.sum(1) + k * aw.sum(1)
    ref['E_depth'] = (om * np.abs(z)).sum(1) + k * (aw * np.abs(z)).sum(1)
    ref['E_rgb'] = ((om[..., None] * col + 4.0 * aw[..., None] * col).sum(1) + k * (aw[..., None] * col).sum(1)
                    + (ref['E_acc'] + 3.0 * np.abs(1.0 - ref['acc']))[:, None] * bg[None, :] / 255.0)
    fw = ETA32 * (np.abs(alpha) * (np.arange(S) + 1.0)[None, :] + np.abs(mask) + 1.0)
    ref['floor_w'] = fw
    ref['floor_acc'] = fw.sum(1)
    ref['floor_depth'] = (fw * np.abs(z)).sum(1)
    ref['floor_rgb'] = (fw[..., None] * col).sum(1) + ref['floor_acc'][:, None] * bg[None, :] / 255.0
    ref['a_s'] = rw['a_s']
    return ref


OUTPUTS = ('rgb', 'acc', 'depth', 'w')


def forward_ratio(got, ref):
    """got: dict with rgb, acc, depth and optionally w -> (per ray max ratio, {output: ratio array}).  inf where an entry of
    E = 0 is not exactly right or a value is not finite."""
    per, n = {}, len(ref['acc'])
    worst = np.zeros(n)
    for k in OUTPUTS:
        if got.get(k) is None:
            continue
        g, want, E, floor = np.asarray(got[k], np.float64), ref[k], ref['E_' + k], ref['floor_' + k]
        assert g.shape == want.shape, (k, g.shape, want.shape)
        err = np.maximum(np.abs(g - want) - floor, 0.0)
        r = np.divide(err, U32 * E, out=np.zeros_like(err), where=E > 0)
        r[(E == 0) & (g != want)] = np.inf
        r[~np.isfinite(g)] = np.inf
        per[k] = r
        worst = np.maximum(worst, r.reshape(n, -1).max(1))
    return worst, per


def term_verdict(term, ref, c_rho):
    """Per ray: (decided [n] bool, ok [n] bool) of a term vector under the margin c_rho [n] u (a_s + a_best)."""
    alpha, a = ref['alpha'], ref['a_s']
    n, S = alpha.shape
    rows = np.arange(n)
    best = ref['term']
    assert np.array_equal(best, np.argmax(alpha, 1))
    lead = alpha[rows, best][:, None] - alpha
    margin = np.asarray(c_rho, np.float64)[:, None] * U32 * (a + a[rows, best][:, None])
    others = np.ones((n, S), bool)
    others[rows, best] = False
    decided = ((lead > margin) | ~others).all(1)
    term = np.asarray(term, np.int64)
    inside = (term >= 0) & (term < S)
    t = np.clip(term, 0, S - 1)
    ok = inside & np.where(decided, term == best, lead[rows, t] <= margin[rows, t])
    return decided, ok


def _name(k, r, per_k):
    if k == 'w':
        return f'ray {r} sample {int(np.argmax(per_k[r]))} weights'
    if k == 'rgb':
        return f'ray {r} rgb[{int(np.argmax(per_k[r]))}]'
    return f'ray {r} {k}'


def check_forward(name, c, got, ref=None, ref32=None):
    """The kernel's (or any) outputs against the float64 truth with the tolerance measured on the fp32 CPU reference, per kind
    of ray; `got`: dict rgb, acc, depth and optionally w, term.  Prints rho_ref / the result's ratio per kind and the share of
    rays whose term the margin leaves undecided; raises naming the worst entry.  -> {kind: (rho_ref, ratio)}."""
    ref = composite_forward_float64(c) if ref is None else ref
    ref32 = forward_torch(c, torch.float32) if ref32 is None else ref32
    rho, _ = forward_ratio(ref32, ref)
    ratio, per = forward_ratio(got, ref)
    assert np.isfinite(rho).all(), f'{name}: the fp32 reference itself breaks an exact entry on rays {np.flatnonzero(~np.isfinite(rho))}'
    base = float(rho[c['groups']['random']].max())
    seen, failures = {}, []
    c_rho = np.zeros(len(rho))
    for kind, rows in c['groups'].items():
        rho_k, got_k = float(rho[rows].max()), float(ratio[rows].max())
        seen[kind] = (rho_k, got_k)
        c_rho[rows] = 4.0 * max(rho_k, base, 1.0)
        if not got_k <= 4.0 * max(rho_k, base, 1.0):
            r = int(rows[np.argmax(ratio[rows])])
            k = max(per, key=lambda kk: per[kk].reshape(len(ratio), -1)[r].max())
            failures.append(f'{kind}: ratio {got_k:.3g} > 4 max(rho_ref {rho_k:.3g}, random rows {base:.3g}, 1) at {_name(k, r, per[k])}')
    line = f'   {name}: rho_ref / result per kind: ' + ', '.join(f'{k} {a:.2g}/{b:.2g}' for k, (a, b) in seen.items())
    if got.get('term') is not None:
        term = np.asarray(got['term'], np.int64)
        decided, ok = term_verdict(term, ref, c_rho)
        rnd = c['groups']['random']
        line += f'; term undecided on {int((~decided[rnd]).sum())} of {len(rnd)} random rays'
        seen['term undecided share'] = float((~decided[rnd]).mean())
        for r in np.flatnonzero(~ok):
            failures.append(f'term of ray {r} is {int(term[r])}, the float64 argmax {int(ref["term"][r])} '
                            f'({"decided" if decided[r] else "undecided, and outside the margin"})')
        for kind, rows in c['groups'].items():
            for r in rows:
                if kind == 'mask=0' and term[r] != 0:
                    failures.append(f'term of the mask = 0 ray {r} is {int(term[r])}, not 0')
                ones = np.flatnonzero(ref['alpha'][r] == 1.0)
                if kind == 'x=25' and len(ones) and term[r] != ones[0]:
                    failures.append(f'term of the saturated ray {r} is {int(term[r])}, not its first alpha = 1 sample {int(ones[0])}')
    print(line)
    assert not failures, f'{name}: ' + '; '.join(failures)
    return seen


# ---- an fp32 numpy forward, and the wrong answers made from it --------------------------------------------------------
MUTANTS = ('scan', 'carry', 'eps', 'last')


def forward_numpy32(c, mutate=None):
    """The forward in np.float32 with a serial transmittance product.  mutate: None; 'ulp' (em of the saturated ray 0 moved by
    one ulp at its middle sample: still right); or one of MUTANTS -- 'scan' (the second chunk's exclusive scan taken
    inclusive), 'carry' (no carry between chunks), 'eps' (1e-10 omitted), 'last' (dist of the last sample 0, not 1e10)."""
    raw, mask, z = (np.asarray(c[k], F32) for k in ('raw', 'mask', 'z'))
    n, S = z.shape
    d = np.asarray(c['rays8'], F32)[:, 3:6]
    dn = np.sqrt((d * d).sum(1, dtype=F32)).astype(F32)
    last = F32(0.0) if mutate == 'last' else F32(1e10)
    dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full((n, 1), last, F32)], 1) * dn[:, None]
    x = raw[..., 3]
    with np.errstate(over='ignore', under='ignore'):
        sp = np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, F32(20.0))))).astype(F32)
        em = np.exp(-(sp * dist)).astype(F32)
        col = (F32(1.0) / (F32(1.0) + np.exp(-raw[..., :3]))).astype(F32)
    if mutate == 'ulp':
        em[0, (S - 1) // 2] = np.nextafter(em[0, (S - 1) // 2], F32(np.inf))
    alpha = ((F32(1.0) - em) * mask).astype(F32)
    tt = (F32(1.0) - alpha) if mutate == 'eps' else ((F32(1.0) - alpha) + F32(1e-10))
    T = np.ones((n, S), F32)
    run = np.ones(n, F32)
    for s in range(S):
        if mutate == 'carry' and s % CHUNK == 0:
            run = np.ones(n, F32)
        T[:, s] = run
        run = (run * tt[:, s]).astype(F32)
        if mutate == 'scan' and CHUNK <= s < 2 * CHUNK:
            T[:, s] = run
    w = (alpha * T).astype(F32)
    acc = w.sum(1, dtype=F32)
    rgb = (w[..., None] * col).sum(1, dtype=F32) + (F32(1.0) - acc)[:, None] * np.asarray(c['bg'], F32)[None, :] / F32(255.0)
    return {'rgb': rgb.astype(F32), 'acc': acc, 'depth': (w * z).sum(1, dtype=F32), 'w': w, 'term': np.argmax(alpha, 1)}
