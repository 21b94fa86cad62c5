"""GPU: the kernels that run once per training step -- pose_motion_bases_kernel and its backward, prior_softmax_kernel,
pack_rays_kernel (occnerf_amd/csrc/preamble.hip), convt3d_col2im / convt3d_im2col and agg_weights_kernel (csrc/train_ops.hip),
point_sdf_backward_kernel (csrc/features.hip), grad_sqnorm_kernel / adam_kernel (csrc/optim.hip) -- PER ENTRY against float64 of
the operands the launch read (tests/step_preamble_restatement.py, with the three kinds of check derived there):

    bit-equal       col2im, im2col, pack_rays, agg_weights' var and rows of equal ids, the pose chain on dyadic operands;
    counted bound   Adam's exp_avg, exp_avg_sq, parameter and gradient norm; the fp64 per-point SDF backward;
    measured c      |got - r| <= c u E with c = 4 max(rho_ref, 1), rho_ref of torch's fp32 CPU evaluation: the pose chain
                    forward and backward, the prior softmax, agg_weights' softmax.

No norm over a tensor, no tolerance relative to the largest entry, no entry left out; what the C ABI writes goes into
over-allocated buffers whose fill must survive.  Each test prints what it saw; the worst values seen on an MI355X stand in the
docstrings."""
import numpy as np
import pytest
import torch

from tests import step_preamble_cases as cases
from tests import step_preamble_restatement as sp

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32


def D(a, dtype=torch.float32):
    """float64 array of values exact in `dtype` -> device tensor."""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)
    out = t.to(dtype)
    assert torch.equal(out.double(), t), 'the case must be exact in its storage format'
    return out.contiguous()


def N(t):
    return t.detach().cpu().numpy()


def _refiner(c):
    from occnerf_amd.modules import BodyPoseRefiner
    dec = BodyPoseRefiner().to(DEV)
    lin = [m for m in dec.block_mlps if isinstance(m, torch.nn.Linear)]
    if c['W'] is not None:
        with torch.no_grad():
            for m, W, b in zip(lin, c['W'], c['b']):
                m.weight.copy_(D(W))
                m.bias.copy_(D(b))
    return dec, lin


def _forward(c, refine):
    from occnerf_amd import ops
    dec, _ = _refiner(c)
    Rs, Ts = ops.pose_motion_bases(dec, D(c['posevec']), refine, D(c['dst_Rs']), D(c['dst_Ts']), D(c['cnl_gtfms']))
    torch.cuda.synchronize()
    return {'Rs': N(Rs), 'Ts': N(Ts)}


# ---- 1. pose chain forward ------------------------------------------------------------------------------------------------
def test_pose_forward_exact_case_is_bit_equal():
    """refine = 0 on signed permutations (a different one per bone) and translations in multiples of 2^-6: the parent table, the
    row / column conventions of the 3x3 inverse and cnl_gtfms @ inverse with no tolerance.
    MI355X: all 216 + 72 entries equal."""
    c = cases.pose_exact_case()
    got, want = _forward(c, False), sp.pose_exact_truth(c)
    sp.check_equal('pose forward exact Rs', got['Rs'], want['Rs'])
    sp.check_equal('pose forward exact Ts', got['Ts'], want['Ts'])


def test_pose_forward_random_without_refinement():
    """refine = 0, rodrigues rotations rounded to fp32, translations about 0.2.
    MI355X: worst error / (u E) 0.84 (rho_ref 0.90, c = 4)."""
    c = cases.pose_random_case()
    rho, worst = sp.check_pose('pose forward refine = 0 random', _forward(c, False), sp.pose_truth(c, False), sp.pose_weights(c, False),
                               sp.pose_ref32(c, False))
    print(f'rho_ref {rho:.3g}, worst {worst:.3g}')


@pytest.mark.parametrize('regime', cases.REGIMES)
def test_pose_forward_refined(regime):
    """refine = 1 in the three regimes of the refiner's last layer: the reference's +-1e-5 initialisation (theta ~ sqrt(1e-5),
    1 - cos(theta) cancels), nn.Linear's default, three zero rows (rvec = 0 for bone 7).
    MI355X: worst error / (u E) 0.78 / 0.47 / 0.56 (rho_ref 0.78 / 0.75 / 1.75, so c = 4 / 4 / 7)."""
    c = cases.pose_case(regime)
    cases.assert_pose_case(c)
    rho, worst = sp.check_pose(f'pose forward {regime}', _forward(c, True), sp.pose_truth(c, True), sp.pose_weights(c, True),
                               sp.pose_ref32(c, True))
    print(f'rho_ref {rho:.3g}, worst {worst:.3g}')


# ---- 2. pose chain backward -----------------------------------------------------------------------------------------------
def _backward(c, dRs, dTs):
    from occnerf_amd import train_ops
    dec, lin = _refiner(c)
    Rs, Ts = train_ops.pose_motion_bases(dec, D(c['posevec']), D(c['dst_Rs']), D(c['dst_Ts']), D(c['cnl_gtfms']))
    params = [m.weight for m in lin] + [m.bias for m in lin]
    gr = torch.autograd.grad([Rs, Ts], params, [D(dRs), D(dTs)])
    torch.cuda.synchronize()
    return {'Rs': N(Rs), 'Ts': N(Ts), 'dW': [N(x) for x in gr[:5]], 'db': [N(x) for x in gr[5:]]}


@pytest.mark.parametrize('regime', cases.REGIMES)
def test_pose_backward_per_entry(regime):
    """All ten gradients (dW[0..4], db[0..4]) against torch's float64 autograd of the modules, dense random cotangents; then the
    exact structure: zero cotangents and a cotangent on the root alone give +-0 everywhere; a cotangent on bone 15, 22 or 23 alone
    leaves every entry of db[4] (= drvec) off the path root -> bone exactly 0 (E = 0 there) and holds the rest to the bound.
    MI355X: dense worst error / (u E) 0.68 / 0.36 / 0.43 (rho_ref 1.01 / 0.47 / 0.68); one bone at most 0.94 / 0.43 / 0.24
    (rho_ref there 0.50 to 1.23); every structural zero exact."""
    c = cases.pose_case(regime)
    cases.assert_pose_case(c)
    args = (c, True, c['dRs'], c['dTs'])
    got = _backward(c, c['dRs'], c['dTs'])
    rho, worst = sp.check_pose(f'pose backward {regime}', got, sp.pose_truth(*args), sp.pose_weights(*args), sp.pose_ref32(*args))
    print(f'dense: rho_ref {rho:.3g}, worst {worst:.3g}')
    for name, (dRs, dTs) in (('zero cotangents', (np.zeros((24, 3, 3)), np.zeros((24, 3)))), ('root only', cases.one_bone_cotangent(c, 0))):
        got = _backward(c, dRs, dTs)
        for k, g in sp.pose_outputs(got):
            assert not g.any(), f'pose backward {regime} {name}: {k} must be +-0 everywhere'
    for bone in cases.PATH_BONES:
        dRs, dTs = cases.one_bone_cotangent(c, bone)
        args = (c, True, dRs, dTs)
        E = sp.pose_weights(*args)
        on = sp.path_to_root(bone)
        off = np.array([b not in on for b in range(1, 24)]).repeat(3)
        assert not E['db'][4][off].any() and E['db'][4][~off].all() and 3 <= len(on) <= 9
        got = _backward(c, dRs, dTs)
        assert not got['db'][4][off].any(), f'pose backward {regime} bone {bone}: drvec off the path root -> {bone} must be exactly 0'
        rho, worst = sp.check_pose(f'pose backward {regime} bone {bone}', got, sp.pose_truth(*args), E, sp.pose_ref32(*args))
        print(f'bone {bone}: rho_ref {rho:.3g}, worst {worst:.3g}')


# ---- 3. prior softmax -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', cases.PRIOR_C)
def test_prior_softmax_per_entry(C):
    """V = 1, 255, 256, 257, 1000; logits in +-30, priors exact 0, 1e-30, random and 1; one voxel with every prior 1e-30 and
    logits near -30.  A prior of 0 gives exactly 0, C = 1 exactly 1.
    MI355X: worst error / (u E) 0 / 0.65 / 0.48 / 0.45 for C = 1 / 2 / 25 / 32 (rho_ref at most 0.65)."""
    from occnerf_amd import ops
    for V in cases.PRIOR_V:
        dec, prior = cases.prior_case(C, V)
        got = ops.prior_softmax(D(dec), D(prior))
        torch.cuda.synchronize()
        assert got.shape == (C, V)
        rho, worst = sp.check_prior_softmax(f'prior_softmax C={C} V={V}', N(got), dec, prior)
        print(f'V={V}: rho_ref {rho:.3g}, worst {worst:.3g}')


# ---- 4. ConvTranspose3d gathers -------------------------------------------------------------------------------------------
def _filled(n, extra=7):
    return torch.full((n + extra,), cases.FILL, device=DEV, dtype=torch.float32)


@pytest.mark.parametrize('shape', cases.CONVT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_convt3d_gathers_are_bit_equal(shape):
    """col2im with and without bias against the np.float32 restatement (bias first, taps kd, kh, kw ascending), im2col against
    the copy-or-zero map, on non-cubic grids; seven fill entries behind each output.
    MI355X: every entry equal at all six shapes."""
    from occnerf_amd import _lib, ops
    Cout, Dd, H, W = shape
    c = cases.convt_case(shape)
    cols, bias, gy = D(c['cols']), D(c['bias']), D(c['gy'])
    total, ctotal = Cout * 8 * Dd * H * W, Cout * 64 * Dd * H * W
    for b in (bias, None):
        out = _filled(total)
        with ops._guard(cols):
            rc = _lib.lib().occnerf_convt3d_col2im(cols.data_ptr(), None if b is None else b.data_ptr(), Cout, Dd, H, W, out.data_ptr(),
                                                   ops._stream(cols))
        _lib.check(rc, 'convt3d_col2im')
        torch.cuda.synchronize()
        o = N(out)
        assert np.all(o[total:] == cases.FILL), f'col2im {shape}: entries behind the output must keep their fill'
        want = sp.col2im(c['cols'], None if b is None else c['bias'], Cout, Dd, H, W)
        sp.check_equal(f'col2im {shape} {"bias" if b is not None else "no bias"}', o[:total].reshape(want.shape), want)
    dcols = _filled(ctotal)
    with ops._guard(gy):
        rc = _lib.lib().occnerf_convt3d_im2col(gy.data_ptr(), Cout, Dd, H, W, dcols.data_ptr(), ops._stream(gy))
    _lib.check(rc, 'convt3d_im2col')
    torch.cuda.synchronize()
    o = N(dcols)
    assert np.all(o[ctotal:] == cases.FILL), f'im2col {shape}: entries behind the output must keep their fill'
    want = sp.im2col(c['gy'].astype(F32), Cout, Dd, H, W)
    sp.check_equal(f'im2col {shape}', o[:ctotal].reshape(want.shape), want)


# ---- 5. agg_weights -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', cases.AGG_K)
def test_agg_weights_per_entry(K):
    """N = 1, 255, 256, 257, 600 over P = 97 counters (1 + Poisson(20), some 1, some 1e6): var bit-equal to the np.float32
    restatement, atts against the float64 softmax of the restated fp32 arguments; the row of equal ids has var = 0 and every
    weight fl(1 / K); rows >= N keep their fill.
    MI355X: var equal everywhere; atts worst error / (u E) 0.24 / 0.31 / 0.30 / 0.16 / 0.15 for K = 2 / 3 / 10 / 39 / 40
    (rho_ref 0.31 / 0.38 / 0.31 / 0.09 / 0.09)."""
    from occnerf_amd import _lib, ops
    for n in cases.AGG_N:
        counter, knn = cases.agg_case(n, K)
        tc, tk = D(counter), torch.from_numpy(knn).to(DEV)
        atts = torch.full((n + 3, K), cases.FILL, device=DEV)
        var = torch.full((n + 3,), cases.FILL, device=DEV)
        with ops._guard(tk):
            rc = _lib.lib().occnerf_agg_weights(tc.data_ptr(), tk.data_ptr(), n, K, atts.data_ptr(), var.data_ptr(), ops._stream(tk))
        _lib.check(rc, 'agg_weights')
        torch.cuda.synchronize()
        a, v = N(atts), N(var)
        assert np.all(a[n:] == cases.FILL) and np.all(v[n:] == cases.FILL), f'agg_weights N={n} K={K}: rows >= N must keep their fill'
        rho, worst = sp.check_agg_weights(f'agg_weights N={n} K={K}', a[:n], v[:n], counter, knn)
        print(f'N={n}: rho_ref {rho:.3g}, worst {worst:.3g}')


# ---- 6. per-point SDF backward --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', cases.SDF_P)
def test_point_sdf_backward_per_entry(P):
    """train_ops._PointSdf with explicit tensors (P = 1: the C ABI over a support set of 8, the 3-NN search needs three points):
    offsets of +-0.02, every fourth row with point_dist = 0 (dir = 0 to its first neighbour, whose contribution is exactly 0),
    both sides of the neg > 1 rule, both signs of c_j; only d_knn_base, only d_dist, and both.  |got - r| <= u |r| + 64 2^-53 B.
    MI355X: worst error / bound 0.98 (the fp32 store)."""
    from occnerf_amd import _lib, ops, train_ops
    c = cases.sdf_case(P)
    base, normals = D(c['base']), torch.from_numpy(c['normals']).to(DEV)
    unit = ops.unit_normals(normals)
    pd = D(c['point_dist']).requires_grad_(True)
    pc_t = (base[:P] + pd.detach()).float().contiguous()
    kidx = ops.knn_small(pc_t, base, 3)
    torch.cuda.synchronize()
    pc = cases.assert_sdf_case(c, N(kidx).astype(np.int64), N(unit))
    assert np.array_equal(pc, N(pc_t))
    d_kb, d_dist = torch.from_numpy(c['d_kb']).to(DEV), D(c['d_dist'])
    for name, use_kb, use_dist in (('both', 1, 1), ('only d_knn_base', 1, 0), ('only d_dist', 0, 1)):
        if P >= 3:
            kb, sdf = train_ops._PointSdf.apply(pd, base, normals, unit)
            outs, grads = ([kb] if use_kb else []) + ([sdf] if use_dist else []), ([d_kb] if use_kb else []) + ([d_dist[:, None]] if use_dist else [])
            got = torch.autograd.grad(outs, [pd], grads)[0]
            assert got.shape == (P, 1)
        else:
            got = torch.full((P + 3,), cases.FILL, device=DEV)
            g_kb, g_dist = (d_kb * use_kb).contiguous(), (d_dist * use_dist).contiguous()      # (alive until the synchronize below)
            with ops._guard(pc_t):
                rc = _lib.lib().occnerf_point_sdf_backward(pc_t.data_ptr(), base.data_ptr(), normals.data_ptr(), unit.data_ptr(), kidx.data_ptr(),
                                                           P, g_kb.data_ptr(), g_dist.data_ptr(), got.data_ptr(), ops._stream(pc_t))
            _lib.check(rc, 'point_sdf_backward')
            torch.cuda.synchronize()
            assert np.all(N(got)[P:] == cases.FILL), 'rows >= P must keep their fill'
            got = got[:P]
        torch.cuda.synchronize()
        g, B = sp.point_sdf_backward_f64(pc, c['base'], c['normals'], N(unit), N(kidx).astype(np.int64), c['d_kb'] * use_kb, c['d_dist'] * use_dist)
        worst = sp.check_point_sdf_backward(f'point_sdf_backward P={P} {name}', N(got).reshape(-1), g, B)
        print(f'{name}: worst {worst:.3g}')


# ---- 7. Adam --------------------------------------------------------------------------------------------------------------
def _off16(n, values):
    """A contiguous tensor of n floats whose data_ptr is 4 bytes past a 16-byte boundary."""
    big = torch.zeros(n + 8, device=DEV)
    t = big[1:1 + n]
    t.copy_(values)
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


@pytest.mark.parametrize('layout', ['aligned', 'parameter off 16 bytes', 'gradient off 16 bytes'])
def test_adam_one_step_per_entry(layout):
    """One FusedAdam step (the third of each tensor: bias corrections of t = 3) at n = 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 5 and
    max_grad_norm None, 1.0, 1e-3: exp_avg, exp_avg_sq and the parameter against float64 of adam1 with the table's fp32 constants
    and the clip coefficient restated from the device's squared norm; grad_norm() against the float64 norm under gamma_266.  A
    parameter (or, alone, a gradient) 4 bytes off 16-byte alignment takes the scalar path of adam_kernel (grad_sqnorm_kernel).
    MI355X: worst error / bound exp_avg 0.963, exp_avg_sq 0.973, p 0.996 in all three layouts (the counts are first-order
    worst cases, and 65 541 entries come close to them); norm at most 0.012 of its bound."""
    from occnerf_amd.optim import FusedAdam
    worst = {}
    for n in cases.adam_sizes():
        c = cases.adam_case(n)
        for mgn in (None, 1.0, 1e-3):
            p0, g0 = D(c['p']), D(c['g'])
            p = (_off16(n, p0) if layout.startswith('parameter') else p0.clone()).detach().requires_grad_(True)
            g = _off16(n, g0) if layout.startswith('gradient') else g0.clone()
            assert (p.data_ptr() % 16 == 4) == layout.startswith('parameter') and (g.data_ptr() % 16 == 4) == layout.startswith('gradient')
            assert p.is_leaf and p.is_contiguous()
            opt = FusedAdam([p], lr=1e-3)
            opt.state[p] = {'step': torch.tensor(2.0), 'exp_avg': D(c['m']), 'exp_avg_sq': D(c['v'])}
            p.grad = g
            opt.step(max_grad_norm=mgn)
            torch.cuda.synchronize()
            st = opt.state[p]
            assert float(st['step']) == 3.0 and np.array_equal(N(g), c['g'].astype(F32)), 'the gradient is read, not written'
            coef = 1.0
            if mgn is not None:
                norm_sq = F32(float(opt._plan['scratch'][0]))
                coef = sp.clip_coef32(norm_sq, mgn)
                norm64 = float(np.sqrt((c['g'] ** 2).sum()))
                nerr = abs(float(opt.grad_norm()) - norm64)
                assert nerr <= sp.grad_norm_bound(norm64), (n, mgn, float(opt.grad_norm()), norm64)
                worst['norm'] = max(worst.get('norm', 0.0), nerr / sp.grad_norm_bound(norm64) if norm64 else 0.0)
            ref = sp.adam_ref(c['p'], c['g'], c['m'], c['v'], coef, sp.adam_constants(1e-3, 3))
            seen = sp.check_adam(f'adam {layout} n={n} max_grad_norm={mgn}', N(p), N(st['exp_avg']), N(st['exp_avg_sq']), ref)
            for k, v in seen.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(layout, {k: round(v, 3) for k, v in worst.items()})


# ---- 8. pack_rays ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', cases.PACK_R)
def test_pack_rays_is_the_gather(R):
    """rays[2,R,3], near, far -> rays8[R,8] under a random permutation and with order = None: bit-equal to the gather.
    MI355X: equal at R = 1, 255, 256, 257."""
    from occnerf_amd import ops
    c = cases.pack_case(R)
    rays, near, far = D(c['rays']), D(c['near']), D(c['far'])
    for order in (c['order'], None):
        got = ops.pack_rays(rays, near, far, None if order is None else torch.from_numpy(order).to(DEV))
        torch.cuda.synchronize()
        sp.check_equal(f'pack_rays R={R} {"permuted" if order is not None else "in order"}', N(got), sp.pack_rays_ref(c['rays'], c['near'], c['far'], order))
