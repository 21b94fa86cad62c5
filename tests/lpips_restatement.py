"""float64 restatements of EVERY launch of the LPIPS kernel set (occnerf_amd/csrc/lpips.hip), the layouts of its two buffers
re-derived from the VGG16 layer table, and the per-entry checks the GPU tests (tests/test_o_lpips_per_entry.py) and the emulated
kernel on the CPU (tests/test_lpips_restatement.py) both go through.  torch, on whatever device the buffers live on; the float64
conv is explicit zero padding, nine shifted slices and one matmul, so it does not rest on a library's float64 conv.

The forward returns its workspace (ops.lpips_forward) and LPIPS.packed() the weight blob: every operand and result of every
launch is a slice of those two tensors.  A check takes the operands exactly as the launch read them (fp32 bits widened), so a
ReLU unit flipped upstream changes the operands of the next check, never its verdict.  With u = 2^-24, gamma_n = n u / (1 - n u):

  scale_in / scale_out   the correctly rounded fp32 quotient, bit for bit (the library is built with -ffp-contract=off and no
                         fast-math flag; a float64 quotient of two fp32 values rounded to fp32 is the correctly rounded one,
                         53 >= 2 * 24 + 2).
  conv3x3 (+ reduce)     r = conv64(input) + b, A = conv64(|input|, |W|) + |b|, e = gamma_{K+2} A + u |r|, K = 9 Cin: the stored value
                         lies in [relu(r - e), relu(r + e)].  Any summation order: split-K and the MFMA's pairing need no case.
                         No term for flushed subnormal products was needed.
  maxpool                bit-equal to the maximum of the four saved inputs.
  head_fwd               first-order propagation, written out at head_forward64.
  head_finish            res: gamma_{hw} mean|respix| + u |r|; val: gamma_5 sum|res|.
  backward               linear in gres once the masks and pool routes are read from the saved fp32 activations (no mask can flip
                         between kernel and reference).  Every term of a result carries the count n of roundings it went
                         through: C_HEAD in head_bwd, 1 per pool merge, 9 Cout + 1 per data gradient (one product rounding, at
                         most 9 Cout - 1 additions in any order, split-K included, and one spare).  S = sum of n |term| is
                         carried beside the absolute chain A = |L_n| ... |L_1| |g|, so |got - r| <= u S / (1 - n_max u) + u |r|:
                         the bound gamma_{sum K_i + c} A of a product of matrices, taken per source tap instead of with the
                         longest path for all (never wider).  It is the bound of the design and it is asserted, but the
                         product of absolute matrices grows by the cancellation of every layer (a factor of 20 to 70 each):
                         measured on the reference alone it is 0.01 |r| for the tap-0 one-hot, 6 |r| for tap 1 and 1e5 ... 1e12 |r|
                         for taps 2 to 4, where it can see no defect at all.  So a second bound with power at every depth is
                         asserted beside it: the error of a result is sum_j c_j e_j, e_j the rounding error one launch made at
                         one of its entries and c_j the coefficient of the exact (signed) maps below it.  |e_j| <= E_j, the
                         worst-case bound of that ONE launch on its real operand (gamma_{9 Cout + 1} conv(|g|, |W|),
                         gamma_{C_HEAD} F for head_bwd, u |g| for a pool merge); under round-to-nearest the e_j are independent
                         with mean zero, so by Hoeffding P(|sum c_j e_j| > LAMBDA sqrt(V)) <= 2 exp(-LAMBDA^2 / 2) with
                         V = sum c_j^2 E_j^2, carried through the chain by the element-wise SQUARED matrices.  LAMBDA = 8:
                         2.5e-14 per entry.  |got - r| <= 8 sqrt(V) + u |r|: in the median 0.004 |r| for the tap-0 one-hot, 0.01 (tap 1),
                         0.04, 0.09 and 0.12 |r| (taps 2 to 4).
"""
import numpy as np
import torch

from tests.trunks_restatement import U, U64, assert_dyadic, check_exact, check_f32, f32_bound, gamma  # noqa: F401

# ---- the layer table: VGG16 features[0:30] as LPIPS cuts it (pretrained_networks.py:96-134) -----------------------------------
BLOCKS = ((2, 64), (2, 128), (3, 256), (3, 512), (3, 512))       # convs per slice, their width; a 2x2 pool in front of slices 2..5
CIN, COUT, POOL_BEFORE, TAP_LAYER = [], [], [], []
for _n, _c in BLOCKS:
    for _j in range(_n):
        CIN.append(COUT[-1] if COUT else 3)
        COUT.append(_c)
        POOL_BEFORE.append(_j == 0 and len(COUT) > 1)
    TAP_LAYER.append(len(COUT) - 1)
LAYERS, TAPS = len(COUT), len(TAP_LAYER)
NUM_CU, BM, BN, BK = 256, 64, 64, 32
EPS = float(np.float32(1e-10))                                      # kEps as the kernels hold it
LAMBDA = 8.0                                                        # Hoeffding factor of the backward's second bound
C_HEAD = 64                                                         # roundings on a term of head_bwd's result, counted below


def round_up(a, b):
    return (a + b - 1) // b * b


def pack_layout():
    """Offsets (floats) of the weight blob: per layer Wf[Kf, Nf], Wd[Kd, Nd], bias; five lins; shift, scale (4 floats each)."""
    p = {k: [] for k in ('wf', 'wd', 'bias', 'kf', 'nf', 'kd', 'nd', 'lin')}
    o = 0
    for l in range(LAYERS):
        kf, nf, kd, nd = round_up(9 * CIN[l], BK), round_up(COUT[l], BN), 9 * COUT[l], round_up(CIN[l], BN)
        for k, v in (('kf', kf), ('nf', nf), ('kd', kd), ('nd', nd)):
            p[k].append(v)
        p['wf'].append(o)
        o += kf * nf
        p['wd'].append(o)
        o += kd * nd
        p['bias'].append(o)
        o += round_up(COUT[l], 4)
    for t in range(TAPS):
        p['lin'].append(o)
        o += COUT[TAP_LAYER[t]]
    p['shift'], p['scale'], p['total'] = o, o + 4, o + 8
    return p


def geometry(H, W):
    hs, ws = [], []
    for l in range(LAYERS):
        if POOL_BEFORE[l]:
            H, W = H // 2, W // 2
        hs.append(H)
        ws.append(W)
    return hs, ws


def splits_for(M, N, K):
    """Split of K over blockIdx.z: two blocks per CU, at least three 32-wide K steps per split, at most 32."""
    tiles = ((M + BM - 1) // BM) * ((N + BN - 1) // BN)
    s = max(1, (2 * NUM_CU) // max(1, tiles))
    return min(s, max(1, (K // BK) // 3), 32)


def forward_splits(N, H, W):
    hs, ws = geometry(H, W)
    return [splits_for(2 * N * hs[l] * ws[l], COUT[l], round_up(9 * CIN[l], BK)) for l in range(LAYERS)]


def backward_splits(nb, H, W):
    """Splits of the 13 data gradients over nb images (nb = N or 2 N)."""
    hs, ws = geometry(H, W)
    return [splits_for(nb * hs[l] * ws[l], CIN[l], 9 * COUT[l]) for l in range(LAYERS)]


def work_layout(N, H, W):
    """Offsets (floats) of the workspace; every region starts on a multiple of 64 floats."""
    hs, ws = geometry(H, W)
    B, o = 2 * N, [0]

    def take(n):
        at = o[0]
        o[0] += round_up(n, 64)
        return at
    w = {'x': take(B * H * W * 3), 'act': [], 'pool': [], 'respix': []}
    gmax, part = B * H * W * 3, 0
    for l in range(LAYERS):
        M = B * hs[l] * ws[l]
        w['act'].append(take(M * COUT[l]))
        gmax = max(gmax, M * COUT[l])
        sf = splits_for(M, COUT[l], round_up(9 * CIN[l], BK))
        if sf > 1:
            part = max(part, sf * M * COUT[l])
        for Md in (M, M // 2):
            sd = splits_for(Md, CIN[l], 9 * COUT[l])
            if sd > 1:
                part = max(part, sd * Md * CIN[l])
        if l + 1 < LAYERS and POOL_BEFORE[l + 1]:
            w['pool'].append(take(B * hs[l + 1] * ws[l + 1] * COUT[l]))
    for t in range(TAPS):
        w['respix'].append(take(N * hs[TAP_LAYER[t]] * ws[TAP_LAYER[t]]))
    w['res'] = take(TAPS * N)
    w['ga'], w['gb'], w['gh'] = take(gmax), take(gmax), take(gmax)
    w['gmax'] = gmax
    w['part'] = take(max(part, 1))
    w['part_floats'] = round_up(max(part, 1), 64)
    w['total'] = o[0]
    return w


def leftover_buffers():
    """Replay of occnerf_lpips_backward's ping-pong: which of 'ga' / 'gb' holds, after it returns, the output of conv1_2's data
    gradient (masked by relu1_1) and which the dx of conv1_1.  'gh' is written last by head_bwd of tap 0."""
    ga, gb = 'ga', 'gb'
    for l in range(LAYERS - 1, -1, -1):                 # conv: ga -> gb
        if l == 0:
            break
        if not POOL_BEFORE[l]:                          # (a pool layer merges gb and gh back into ga: no swap)
            ga, gb = gb, ga
    return ga, gb                                       # (conv1_1's input, conv1_1's output)


# ---- views ------------------------------------------------------------------------------------------------------------------
def unpack(packed):
    """The regions of the weight blob as views: Wf[l][Kf, Nf], Wd[l][Kd, Nd], bias[l][Cout], lin[t][C], shift[3], scale[3]."""
    p = pack_layout()
    assert packed.numel() == p['total']
    v = {'Wf': [], 'Wd': [], 'bias': [], 'lin': []}
    for l in range(LAYERS):
        v['Wf'].append(packed[p['wf'][l]:p['wf'][l] + p['kf'][l] * p['nf'][l]].view(p['kf'][l], p['nf'][l]))
        v['Wd'].append(packed[p['wd'][l]:p['wd'][l] + p['kd'][l] * p['nd'][l]].view(p['kd'][l], p['nd'][l]))
        v['bias'].append(packed[p['bias'][l]:p['bias'][l] + COUT[l]])
    for t in range(TAPS):
        v['lin'].append(packed[p['lin'][t]:p['lin'][t] + COUT[TAP_LAYER[t]]])
    v['shift'], v['scale'] = packed[p['shift']:p['shift'] + 3], packed[p['scale']:p['scale'] + 3]
    return v


def pack_expected(conv_w, conv_b, lins, shift, scale):
    """The same regions from the module's weights by permutation in torch (padding rows and columns zero)."""
    p = pack_layout()
    v = {'Wf': [], 'Wd': [], 'bias': [], 'lin': [t.detach().reshape(-1).float() for t in lins],
         'shift': shift.detach().reshape(3).float(), 'scale': scale.detach().reshape(3).float()}
    for l in range(LAYERS):
        w = conv_w[l].detach().float()
        assert tuple(w.shape) == (COUT[l], CIN[l], 3, 3)
        wf = torch.zeros(p['kf'][l], p['nf'][l], dtype=torch.float32, device=w.device)
        wf[:9 * CIN[l], :COUT[l]] = w.permute(2, 3, 1, 0).reshape(9 * CIN[l], COUT[l])                  # [(ky, kx, ci), co]
        wd = torch.zeros(p['kd'][l], p['nd'][l], dtype=torch.float32, device=w.device)
        wd[:, :CIN[l]] = w.flip(2, 3).permute(2, 3, 0, 1).reshape(9 * COUT[l], CIN[l])                  # W[co, ci, 2-ky, 2-kx]
        v['Wf'].append(wf)
        v['Wd'].append(wd)
        v['bias'].append(conv_b[l].detach().float())
    return v


def blob(regions):
    """pack_expected's regions laid out as the flat blob (gaps zero)."""
    p = pack_layout()
    out = torch.zeros(p['total'], dtype=torch.float32, device=regions['shift'].device)
    pv = unpack(out)
    for k in ('Wf', 'Wd', 'bias', 'lin'):
        for dst, src in zip(pv[k], regions[k]):
            dst.copy_(src)
    pv['shift'].copy_(regions['shift'])
    pv['scale'].copy_(regions['scale'])
    return out


def views(work, N, H, W):
    """The regions of the workspace as NHWC views: x[2N,H,W,3], act[l][2N,h,w,Cout], pool[k], respix[t][N,hw], res[5,N], and the
    three gradient buffers ga / gb / gh flat."""
    wl = work_layout(N, H, W)
    assert work.numel() == wl['total'], (work.numel(), wl['total'])
    hs, ws = geometry(H, W)
    B = 2 * N

    def cut(at, *shape):
        return work[at:at + int(np.prod(shape))].view(*shape)
    v = {'N': N, 'H': H, 'W': W, 'x': cut(wl['x'], B, H, W, 3), 'act': [], 'pool': [], 'respix': []}
    for l in range(LAYERS):
        v['act'].append(cut(wl['act'][l], B, hs[l], ws[l], COUT[l]))
        if l + 1 < LAYERS and POOL_BEFORE[l + 1]:
            v['pool'].append(cut(wl['pool'][len(v['pool'])], B, hs[l + 1], ws[l + 1], COUT[l]))
    for t in range(TAPS):
        l = TAP_LAYER[t]
        v['respix'].append(cut(wl['respix'][t], N, hs[l] * ws[l]))
    v['res'] = cut(wl['res'], TAPS, N)
    for k in ('ga', 'gb', 'gh'):
        v[k] = cut(wl[k], wl['gmax'])
    return v


def conv_input(v, l):
    """The tensor layer l's forward conv read."""
    if l == 0:
        return v['x']
    return v['pool'][sum(POOL_BEFORE[:l + 1]) - 1] if POOL_BEFORE[l] else v['act'][l - 1]


# ---- float64 of one launch ------------------------------------------------------------------------------------------------------
def np64(t):
    return t.detach().double().cpu().numpy()


def im2col(x):
    """[B,H,W,C] -> [B H W, 9 C], k = (ky 3 + kx) C + c holding x[b, y+ky-1, x+kx-1, c], zero outside."""
    B, H, W, C = x.shape
    p = torch.zeros(B, H + 2, W + 2, C, dtype=x.dtype, device=x.device)
    p[:, 1:-1, 1:-1] = x
    return torch.cat([p[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], 3).reshape(B * H * W, 9 * C)


def conv64(x, Wm, bias=None, xabs=None):
    """-> r, A [B,H,W,Co] in float64: r = im2col(x) Wm + b, A = im2col(|x|) |Wm| + |b| (xabs: the absolute operand, if not |x|)."""
    B, H, W, _ = x.shape
    Wm = Wm.double()
    r = im2col(x.double()) @ Wm
    A = im2col(x.double().abs() if xabs is None else xabs) @ Wm.abs()
    if bias is not None:
        r, A = r + bias.double(), A + bias.double().abs()
    return r.view(B, H, W, -1), A.view(B, H, W, -1)


def pool_windows(a):
    """[B,h,w,C] -> the four inputs of every 2x2/2 window in row-major order, each [B,h/2,w/2,C] (floored)."""
    h2, w2 = a.shape[1] // 2, a.shape[2] // 2
    return [a[:, dy:2 * h2:2, dx:2 * w2:2] for dy in (0, 1) for dx in (0, 1)]


def first_max(q):
    """-> (max, index of the FIRST maximum in row-major order), by the kernels' own strict comparisons."""
    m, arg = q[0], torch.zeros_like(q[0], dtype=torch.int64)
    for i in range(1, 4):
        gt = q[i] > m
        m, arg = torch.where(gt, q[i], m), torch.where(gt, torch.full_like(arg, i), arg)
    return m, arg


def pool_route(act, gp):
    """The pool's gradient gp[B,h/2,w/2,C] sent to the first maximum of each window of act[B,h,w,C]; an odd last row or column
    gets none."""
    B, h, w, C = act.shape
    h2, w2 = h // 2, w // 2
    _, arg = first_max(pool_windows(act))
    out = torch.zeros(B, h, w, C, dtype=gp.dtype, device=gp.device)
    for i in range(4):
        out[:, i // 2:2 * h2:2, i % 2:2 * w2:2] = torch.where(arg == i, gp, torch.zeros_like(gp))
    return out


def _norms(f, eps):
    n = torch.sqrt((f * f).sum(-1, keepdim=True) + eps)
    return n, n + eps


def head_forward64(act, N, lin, eps=EPS):
    """respix of one tap from its activations act[2N,h,w,C] -> r[N,hw], bound[N,hw].

    Kernel: s = sum a^2 (fma chain + 6 cross-lane additions), d0 = sqrt(s + eps) + eps, q = a / d0, d = q0 - q1,
    r = sum lin d^2.  First order, with every sum taken in any order: s carries gamma_C (C products and additions) and one more
    for + eps; the square root halves that and adds one rounding, + eps another: e_d = gamma_{C+1} / 2 + 2 u relative on d0.
    q: e_q = e_d + u.  d: |delta d| <= e_q (|q0| + |q1|) + u |d|.  d^2: 2 |d| |delta d| + u d^2.  The lin sum: gamma_{C+4} on
    sum lin d^2 (C products and additions, the 6 cross-lane ones and spare).  A factor 1.01 covers the second-order terms."""
    C = act.shape[-1]
    a, b = act[:N].double().reshape(N, -1, C), act[N:].double().reshape(N, -1, C)
    lin = lin.double()
    (_, d0), (_, d1) = _norms(a, eps), _norms(b, eps)
    q0, q1 = a / d0, b / d1
    d = q0 - q1
    r = (lin * d * d).sum(-1)
    e_q = gamma(C + 1) / 2 + 3 * U
    dd = e_q * (q0.abs() + q1.abs()) + U * d.abs()
    bound = 1.01 * ((lin.abs() * (2 * d.abs() * dd + U * d * d)).sum(-1) + gamma(C + 4) * (lin.abs() * d * d).sum(-1)) + U * r.abs()
    return r, bound


def head_backward64(act, N, lin, gres_t, need0, need1, eps=EPS):
    """head_bwd of one tap -> g, A, F, each [nb,h,w,C] over the images wanted (in0's first).

    g0 = [a > 0] (u / d0 - k0 a), g1 = [b > 0] (-u / d1 + k1 b) with coef = gres / hw, u = 2 coef lin (a / d0 - b / d1),
    k0 = sum(u a) / (d0^2 n0).  A is the absolute form |u| / d + |k| |a| the chain carries.  F is the full absolute form, with
    |q0| + |q1| in place of |d| inside u and sum |u| |a| inside k: what a per-entry bound on this launch alone needs, because
    d and the dot product are themselves sums that may cancel.

    C_HEAD, roundings on one term of g0 (J = C / 64 <= 8 channels per lane): n0 = sqrt(s + eps): (J + 6 + 1) / 2 + 1 <= 8.5;
    d0 = n0 + eps: 10; coef: 1; q = a / d0: 11; d: 12; u (two products, the 2 is exact): 15; u / d0: 26; dot (J fma + 6
    cross-lane): 29; d0 d0 n0: 31; k0: 61; k0 a: 62; the difference: 63.  64."""
    B, h, w, C = act.shape
    a, b = act[:N].double().reshape(N, -1, C), act[N:].double().reshape(N, -1, C)
    lin = lin.double()
    (n0, d0), (n1, d1) = _norms(a, eps), _norms(b, eps)
    coef = (gres_t.double() / (h * w)).view(N, 1, 1)
    q0, q1 = a / d0, b / d1
    u = 2 * coef * lin * (q0 - q1)
    uF = 2 * coef.abs() * lin.abs() * (q0.abs() + q1.abs())
    out = []
    for need, f, n, d, sign in ((need0, a, n0, d0, 1.0), (need1, b, n1, d1, -1.0)):
        if not need:
            continue
        k = (u * f).sum(-1, keepdim=True) / (d * d * n)
        kF = (uF * f.abs()).sum(-1, keepdim=True) / (d * d * n)
        live = f > 0
        z = torch.zeros_like(f)
        out.append((torch.where(live, sign * (u / d - k * f), z), torch.where(live, u.abs() / d + k.abs() * f.abs(), z),
                    torch.where(live, uF / d + kF * f.abs(), z)))
    return tuple(torch.cat([o[i] for o in out]).view(-1, h, w, C) for i in range(3))


def forward64(pk, in0, in1, eps=EPS):
    """The whole forward in float64 from the packed regions pk and NCHW images: a state like views() (float64 tensors), + val."""
    N, _, H, W = in0.shape
    x = torch.cat([in0, in1]).double().permute(0, 2, 3, 1)
    x = (x - pk['shift'].double()) / pk['scale'].double()
    v = {'N': N, 'H': H, 'W': W, 'x': x, 'act': [], 'pool': [], 'respix': []}
    for l in range(LAYERS):
        if POOL_BEFORE[l]:
            x = first_max(pool_windows(x))[0]
            v['pool'].append(x)
        x = torch.relu(conv64(x, pk['Wf'][l][:9 * CIN[l], :COUT[l]], pk['bias'][l])[0])
        v['act'].append(x)
    for t in range(TAPS):
        v['respix'].append(head_forward64(v['act'][TAP_LAYER[t]], N, pk['lin'][t], eps)[0])
    v['res'] = torch.stack([r.mean(1) for r in v['respix']])
    v['val'] = v['res'].sum(0)
    return v


def backward64_state(v, pk, gres, need0, need1, eps=EPS):
    """The backward as a linear map of gres[5,N] on the saved state v (views() of a workspace, or forward64's float64 state).
    -> dict: dx, A, S, V [nb,H,W,3] (gradient wrt the scaled image x, its absolute chain, its rounding-weighted chain, the
    sum of squared local bounds through the squared maps), n_max,
    gh (head_bwd of tap 0: g, A, F), g11 (the masked output of conv1_2's data gradient), b0, nb."""
    N = v['N']
    b0, nb = (0 if need0 else N), (int(bool(need0)) + int(bool(need1))) * N
    gres = gres.double()
    act = [a[b0:b0 + nb] for a in v['act']]
    top = max([t for t in range(TAPS) if bool((gres[t] != 0).any())] or [0])     # taps above carry exact zeros
    g, A, F = head_backward64(v['act'][TAP_LAYER[top]], N, pk['lin'][top], gres[top], need0, need1, eps)
    S, n_max = C_HEAD * A, C_HEAD
    V = (gamma(C_HEAD) * F) ** 2
    out = {'b0': b0, 'nb': nb, 'gh': (g, A, F)}
    t = top - 1
    for l in range(TAP_LAYER[top], -1, -1):
        Wd = pk['Wd'][l][:, :CIN[l]]
        K = 9 * COUT[l] + 1
        r, A2 = conv64(g, Wd, xabs=A)
        S = im2col(S) @ Wd.double().abs()
        S = S.view(A2.shape) + K * A2
        E = gamma(K) * (im2col(g.abs()) @ Wd.double().abs())
        V = (im2col(V) @ (Wd.double() ** 2) + E * E).view(A2.shape)
        n_max += K
        if l > 0 and not POOL_BEFORE[l]:
            live = act[l - 1] > 0
            z = torch.zeros_like(r)
            r, A2, S, V = torch.where(live, r, z), torch.where(live, A2, z), torch.where(live, S, z), torch.where(live, V, z)
        if l == 1:
            out['g11'] = r
        if l == 0:
            break
        if POOL_BEFORE[l]:
            gh, Ah, Fh = head_backward64(v['act'][l - 1], N, pk['lin'][t], gres[t], need0, need1, eps)
            if t == 0:
                out['gh'] = (gh, Ah, Fh)
            t -= 1
            live = act[l - 1] > 0
            z = torch.zeros_like(gh)
            g = torch.where(live, gh + pool_route(act[l - 1], r), z)
            A = torch.where(live, Ah + pool_route(act[l - 1], A2), z)
            S = torch.where(live, C_HEAD * Ah + pool_route(act[l - 1], S) + A, z)
            V = torch.where(live, (gamma(C_HEAD) * Fh) ** 2 + pool_route(act[l - 1], V) + (U * g) ** 2, z)
            n_max += 1
        else:
            g, A = r, A2
    out.update(dx=r, A=A2, S=S, V=V, n_max=n_max)
    return out


def backward64(work, packed, gres, need0, need1, N, H, W):
    return backward64_state(views(work, N, H, W), unpack(packed), gres, need0, need1)


# ---- checks ---------------------------------------------------------------------------------------------------------------------
class EntryError(AssertionError):
    """A per-entry check failed: .check is its name, .bad the mask of the failing entries."""

    def __init__(self, msg, check, bad):
        super().__init__(msg)
        self.check, self.bad = check, bad


def check_bound(name, got, r, bound):
    """|got - r| <= bound per entry (zero-bound entries exact; a NaN fails).  -> worst err / bound."""
    got, r, bound = np.asarray(got, np.float64), np.asarray(r, np.float64), np.asarray(bound, np.float64)
    assert got.shape == r.shape == bound.shape, (name, got.shape, r.shape, bound.shape)
    err = np.abs(got - r)
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise EntryError(f'{name}: {int(bad.sum())}/{bad.size} entries beyond the bound, first at {i}: got {got[i]!r}, '
                         f'want {r[i]!r}, bound {bound[i]:.3e}', name, bad)
    pos = bound > 0
    return float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0


def relu_interval(r, A, n):
    """-> lo, hi: what a ReLU epilogue may store when the pre-activation is r within gamma_n A + u |r| (ReLU is monotone)."""
    e = f32_bound(r, A, n)
    return np.maximum(r - e, 0.0), np.maximum(r + e, 0.0)


def single_valued(lo, hi):
    """Entries whose [lo, hi] holds exactly one fp32 value."""
    a, b = lo.astype(np.float32), hi.astype(np.float32)
    a = np.where(a.astype(np.float64) < lo, np.nextafter(a, np.float32(np.inf)), a)          # the smallest fp32 >= lo
    b = np.where(b.astype(np.float64) > hi, np.nextafter(b, np.float32(-np.inf)), b)         # the largest fp32 <= hi
    return a == b


def interval_outside(got, lo, hi):
    return ~((lo <= got) & (got <= hi))


def check_relu_interval(name, got, r, A, n):
    """got in [relu(r - e), relu(r + e)] per entry.  -> worst |got - relu(r)| / e."""
    got, r, A = np.asarray(got, np.float64), np.asarray(r, np.float64), np.asarray(A, np.float64)
    assert got.shape == r.shape, (name, got.shape, r.shape)
    lo, hi = relu_interval(r, A, n)
    bad = interval_outside(got, lo, hi)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise EntryError(f'{name}: {int(bad.sum())}/{bad.size} entries outside [lo, hi], first at {i}: got {got[i]!r}, '
                         f'lo {lo[i]!r}, hi {hi[i]!r}, r {r[i]!r}', name, bad)
    e = f32_bound(r, A, n)
    return float(np.max(np.abs(got - np.maximum(r, 0.0)) / np.where(e > 0, e, 1.0)))


def fp32_quotient(num, den):
    """The correctly rounded fp32 quotient of fp32 arrays (through float64: innocuous double rounding, 53 >= 2 * 24 + 2)."""
    return (np.asarray(num, np.float32).astype(np.float64) / np.asarray(den, np.float32).astype(np.float64)).astype(np.float32)


def nhwc_of(t):
    """A logical [N,3,H,W] tensor -> float32 numpy [N,H,W,3]."""
    return t.detach().float().permute(0, 2, 3, 1).cpu().numpy()


def worst(seen, kind, ratio):
    seen[kind] = max(seen.get(kind, 0.0), float(ratio))


def check_forward(work, packed, in0, in1, val, res, layers=None, taps=None, dyadic_layers=(), seen=None):
    """Every launch of one forward against float64 of its own input as it lies in the workspace.  layers / taps: the part to
    check (default: everything).  dyadic_layers: layers whose result must ALSO be bit-equal to float64 (assert_dyadic on the
    reference).  -> {kernel kind: worst err / bound}."""
    N, _, H, W = in0.shape
    v, pk = views(work, N, H, W), unpack(packed)
    seen = {} if seen is None else seen
    layers = range(LAYERS) if layers is None else layers
    taps = range(TAPS) if taps is None else taps
    splits = forward_splits(N, H, W)
    # scale_in
    img = np.concatenate([nhwc_of(in0), nhwc_of(in1)])
    shift, scale = pk['shift'].cpu().numpy(), pk['scale'].cpu().numpy()
    check_exact('scale_in', np64(v['x']), fp32_quotient(img - shift, np.broadcast_to(scale, img.shape)))
    worst(seen, 'scale_in', 0.0)
    for l in layers:
        if POOL_BEFORE[l]:
            k = sum(POOL_BEFORE[:l + 1]) - 1
            check_exact(f'maxpool {k}', np64(v['pool'][k]), np64(first_max(pool_windows(v['act'][l - 1]))[0]))
            worst(seen, 'maxpool', 0.0)
        r, A = conv64(conv_input(v, l), pk['Wf'][l][:9 * CIN[l], :COUT[l]], pk['bias'][l])
        r, A, got = np64(r), np64(A), np64(v['act'][l])
        kind = 'conv3x3<%s> %s' % ('true' if CIN[l] % BK else 'false', 'splits == 1' if splits[l] == 1 else 'splits > 1')
        worst(seen, kind, check_relu_interval(f'conv {l} ({kind})', got, r, A, 9 * CIN[l] + 2))
        if l in dyadic_layers:
            q = 128.0                                       # images in 1/8, weights in 1/4, twice
            assert_dyadic(f'conv {l}', r * q, A * q)
            check_exact(f'conv {l} dyadic', got, np.maximum(r, 0.0))
    for t in taps:
        r, bound = head_forward64(v['act'][TAP_LAYER[t]], N, pk['lin'][t])
        worst(seen, 'head_fwd', check_bound(f'head_fwd {t}', np64(v['respix'][t]), np64(r), np64(bound)))
    if res is not None and list(taps) == list(range(TAPS)):
        for t in range(TAPS):
            rp = np64(v['respix'][t])
            hw = rp.shape[1]
            worst(seen, 'head_finish res', check_f32(f'res {t}', np64(res[t])[None], rp.mean(1)[None], np.abs(rp).mean(1)[None], hw))
        rr = np64(res)
        worst(seen, 'head_finish val', check_f32('val', np64(val.reshape(-1))[None], rr.sum(0)[None], np.abs(rr).sum(0)[None], 5))
    return seen


def check_backward(work, packed, gres, need0, need1, d0, d1, shape, leftovers=True, seen=None, name=''):
    """d_in0 / d_in1 (logical [N,3,H,W], or None) of one backward per entry against the float64 map on the saved state, and the
    three buffers that survive it, each from the operands its launch read.  -> {kernel kind: worst err / bound}."""
    N, _, H, W = shape
    v, pk = views(work, N, H, W), unpack(packed)
    seen = {} if seen is None else seen
    ref = backward64_state(v, pk, gres, need0, need1)
    b0, nb = ref['b0'], ref['nb']
    scale = pk['scale'].double()
    got = np.concatenate([nhwc_of(d) for d in (d0, d1) if d is not None]).astype(np.float64)
    assert (d0 is not None) == bool(need0) and (d1 is not None) == bool(need1)
    if leftovers:
        _check_leftovers(v, pk, ref, gres, got, N, H, W, seen, name)
    r = np64(ref['dx'] / scale)
    bound = np64(ref['S'] / scale) * U / (1 - ref['n_max'] * U) + ref['n_max'] * U64 * np64(ref['A'] / scale) + U * np.abs(r)
    worst(seen, 'backward chain (worst case)', check_bound(f'{name} d_in', got, r, bound))
    worst(seen, 'backward chain (Hoeffding)', check_bound(f'{name} d_in', got, r, LAMBDA * np64(torch.sqrt(ref['V']) / scale) + U * np.abs(r)))
    return seen


def _check_leftovers(v, pk, ref, gres, got, N, H, W, seen, name):
    """The three buffers that survive occnerf_lpips_backward, each against float64 of the operands its launch read."""
    b0, nb = ref['b0'], ref['nb']
    hs, ws = geometry(H, W)
    in_buf, out_buf = leftover_buffers()
    # head_bwd of tap 0 from the saved act[1]: gh, full-batch indexing
    g, _, F = ref['gh']
    gh = v['gh'][:2 * N * H * W * 64].view(2 * N, H, W, 64)[b0:b0 + nb]
    worst(seen, 'head_bwd', check_f32(f'{name} head_bwd 0', np64(gh), np64(g), np64(F), C_HEAD))
    # conv1_1's data gradient from conv1_2's saved (masked) output
    g11 = v[in_buf][:2 * N * H * W * 64].view(2 * N, H, W, 64)[b0:b0 + nb]
    dx = v[out_buf][:2 * N * H * W * 3].view(2 * N, H, W, 3)[b0:b0 + nb]
    rr, AA = conv64(g11, pk['Wd'][0][:, :3])
    sp = backward_splits(nb, H, W)[0]
    worst(seen, 'dgrad conv1_1 ' + ('splits == 1' if sp == 1 else 'splits > 1'),
          check_f32(f'{name} dgrad conv1_1', np64(dx), np64(rr), np64(AA), 9 * 64 + 2))
    assert not bool(g11[v['act'][0][b0:b0 + nb] <= 0].any()), f'{name}: conv1_2 data gradient must be zero where relu1_1 is'
    # scale_out: the exact quotient of the dx it read
    dxn = dx.cpu().numpy()
    check_exact(f'{name} scale_out', got, fp32_quotient(dxn, np.broadcast_to(pk['scale'].cpu().numpy(), dxn.shape)))
    worst(seen, 'scale_out', 0.0)
