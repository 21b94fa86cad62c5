"""GPU: the render-path feature kernels of occnerf_amd/csrc/features.hip PER ENTRY against their restatement
(tests/features_restatement.py, with the counted bounds derived there) on the seeded inputs of tests/features_cases.py.

Covered, through the C ABI (occnerf_sample_features_centered, occnerf_point_table, occnerf_point_pack):

    sample_features_kernel                       nscale 1..4, att_in / geo_idxs given or not, N = 1, 255, 256, 257, host offsets given
                                                 and NULL (every level through the generic index path)
    sample_features8_kernel<false, false>        standard layout, 256-thread blocks: N < 6144, or P = 9217 at any N
    sample_features8_kernel<false, true>         standard layout, the block-wide LDS image: P <= 9216 and N >= 6144
    sample_features8_kernel<true, false | true>  the last level hashed with a size that is no power of two, both forms
    point_table_kernel, point_pack_kernel        P = 1, 255, 256, 257

    bit-equal   the signed distance, the encoder input x, the 32 encoded columns (zero for x outside [0, 1]), the variance in each
                kernel's own order, columns 0..35 of a row of equal counts, rows of equal (ids, counts) among each other, one
                sample in all 8 slots of a trip, a row list against the whole-array run, the centre path against the plain one,
                the table rows and the pack records;
    bounded     columns 0..34: |got - sum_j r_j t_j| <= ((1 + ew)(1 + gamma_acc) - 1) sum_j |r_j t_j| per entry, r the float64
                softmax of the bit-exact arguments.

No norm over a tensor, no tolerance relative to the largest entry, no entry left out.  mlp_in, raw, enc_in, the table and the pack
records are followed by 256 bytes of fill that must survive; raw's columns 0..3 and every row at or beyond a list's count keep
their fill.  Each test prints what it saw; the worst values seen on an MI355X stand in the docstrings."""
import numpy as np
import pytest
import torch

from tests import features_cases as cases
from tests import features_restatement as fr
from tests.gpu_util import T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FILL, PAD = -7.5, 64                                      # 64 floats: 256 bytes behind every buffer
_memo = {}


def _form(P, n):
    return 'LDS form' if P <= cases.LDS_POINTS and n >= cases.LDS_MIN_N else '256-thread form'


def _filled(n):
    return torch.full((n + PAD,), FILL, device=DEV)


def _layout_dev(generic):
    key = ('lay', generic)
    if key not in _memo:
        lay = cases.layout(generic)
        h_off = np.ascontiguousarray(lay['offsets'], np.int32)
        _memo[key] = {'emb': T(lay['emb']), 'off': T(h_off), 'h_off': h_off, 'S': lay['S'], 'H': lay['H']}
    return _memo[key]


def _point_table(P):
    """occnerf_point_table on the first P points of the 257-point model -> the [P, 64] device rows, checked per entry."""
    from occnerf_amd import _lib, ops
    m, ld = cases.model(), _layout_dev(False)
    kb, sdf, learn = T(m['knn_base'][:P]), T(m['sdf'][:P]), T(m['learnable'][:P])
    table = _filled(P * 64)
    with ops._guard(kb):
        rc = _lib.lib().occnerf_point_table(kb.data_ptr(), sdf.data_ptr(), learn.data_ptr(), P, m['bound'], m['two_bound'], ld['emb'].data_ptr(),
                                            ld['off'].data_ptr(), ld['h_off'].ctypes.data, 16, ld['S'], ld['H'], table.data_ptr(), ops._stream(kb))
    _lib.check(rc, 'point_table')
    torch.cuda.synchronize()
    t = table.cpu().numpy()
    assert np.all(t[P * 64:] == FILL), f'point_table P = {P}: the fill behind the table must survive'
    rows = t[:P * 64].reshape(P, 64)
    assert np.all(rows[:, 36:] == FILL), f'point_table P = {P}: the columns beyond 36 of a 64-float row are not the kernel\'s'
    want = m['table'][:P]
    ne = fr.bits(rows[:, :36]) != fr.bits(want)
    assert not ne.any(), f'point_table P = {P}: {int(ne.sum())} entries are not bit-equal; first at point {np.argwhere(ne)[0][0]} column {np.argwhere(ne)[0][1]}'
    zero = ((m['table_x'][:P] < 0) | (m['table_x'][:P] > 1)).any(1)
    assert not rows[zero, :32].any() and not rows[:, 35].any() and np.array_equal(fr.bits(rows[:, 32:35]), fr.bits(m['learnable'][:P]))
    return table[:P * 64].reshape(P, 64), int(zero.sum())


def _model_dev(P):
    """Device copies of a model; the 257-point model's table is the one occnerf_point_table wrote (zero beyond column 36)."""
    key = ('model', P)
    if key not in _memo:
        m = cases.model(P)
        if P == 257:
            table = _point_table(P)[0].clone()
            table[:, 36:] = 0.0
        else:
            table = T(cases.table64(m['table']))
        d = {'base': T(m['base']), 'normals': T(m['normals']), 'unit': T(m['unit']), 'counter': T(m['counter']), 'table': table.contiguous(), 'P': P}
        d['geo'], d['tail'] = _point_pack(d, m, table.cpu().numpy())
        _memo[key] = d
    return _memo[key]


def _point_pack(d, m, table_np):
    from occnerf_amd import _lib, ops
    P = d['P']
    geo, tail = _filled(P * 16), _filled(P * 4)
    with ops._guard(d['base']):
        rc = _lib.lib().occnerf_point_pack(d['base'].data_ptr(), d['normals'].data_ptr(), d['unit'].data_ptr(), d['counter'].data_ptr(),
                                           d['table'].data_ptr(), P, geo.data_ptr(), tail.data_ptr(), ops._stream(d['base']))
    _lib.check(rc, 'point_pack')
    torch.cuda.synchronize()
    want_geo, want_tail = fr.pack_records({k: v[:P] if isinstance(v, np.ndarray) else v for k, v in m.items()}, table_np[:, :36])
    g, t = geo.cpu().numpy(), tail.cpu().numpy()
    assert np.all(g[P * 16:] == FILL) and np.all(t[P * 4:] == FILL), f'point_pack P = {P}: the fill behind the records must survive'
    assert np.array_equal(fr.bits(g[:P * 16]).reshape(P, 16), fr.bits(want_geo)), f'point_pack P = {P}: the 64-byte geo records are not copies'
    assert np.array_equal(fr.bits(t[:P * 4]).reshape(P, 4), fr.bits(want_tail)), f'point_pack P = {P}: (table columns 32..34, count) are not copies'
    return geo[:P * 16].reshape(P, 16).contiguous(), tail[:P * 4].reshape(P, 4).contiguous()


def _call(P, generic, xyz, knn, nscale=4, rows=None, count=None, geo_idxs=None, att_in=None, pack=True, h_given=True,
          counter=True, center=None, center_agg=None, whole=False):
    """One launch through the C ABI into filled buffers.  xyz, knn: numpy or device tensors; rows: int32 [cap] with count.
    -> (mlp_in [n, 68], dist [n], x [n, 4]) numpy, n = the count (or N); with whole=True the three device buffers."""
    from occnerf_amd import _lib, ops
    d, ld = _model_dev(P), _layout_dev(generic)
    dev = lambda a: None if a is None else (a if torch.is_tensor(a) else T(a))       # noqa: E731
    xyz, knn, rows, geo_idxs, att_in = dev(xyz), dev(knn), dev(rows), dev(geo_idxs), dev(att_in)
    cap = xyz.shape[0] if rows is None else rows.shape[0]
    n = cap if count is None else int(count)
    n_dev = None if count is None else T(np.array([count], np.int32))
    mlp_in, raw, enc = _filled(cap * 68), _filled(cap * 5), _filled(cap * 4)
    ptr = lambda t: None if t is None else t.data_ptr()                            # noqa: E731
    with ops._guard(xyz):
        rc = _lib.lib().occnerf_sample_features_centered(
            xyz.data_ptr(), cap, knn.data_ptr(), nscale, d['base'].data_ptr(), d['normals'].data_ptr(), d['unit'].data_ptr(),
            d['counter'].data_ptr() if counter else None, d['table'].data_ptr(), cases.b32()[0], cases.b32()[1], ld['emb'].data_ptr(),
            ld['off'].data_ptr(), ld['h_off'].ctypes.data if h_given else None, 16, ld['S'], ld['H'], ptr(geo_idxs), ptr(att_in), ptr(rows),
            ptr(n_dev), d['geo'].data_ptr() if pack else None, d['tail'].data_ptr() if pack else None, P if pack else 0, ptr(center),
            ptr(center_agg), mlp_in.data_ptr(), raw.data_ptr(), enc.data_ptr(), ops._stream(xyz))
    _lib.check(rc, 'sample_features')
    torch.cuda.synchronize()
    for name, buf, w in (('mlp_in', mlp_in, 68), ('raw', raw, 5), ('enc_in', enc, 4)):
        assert bool((buf[n * w:] == FILL).all()), f'{name}: the rows from {n} on and the 256 bytes behind the buffer must keep their fill'
    assert bool((raw[:cap * 5].view(cap, 5)[:, :4] == FILL).all()), 'raw: columns 0..3 are not this kernel\'s'
    if whole:
        return mlp_in, raw, enc
    return (mlp_in[:n * 68].view(n, 68).cpu().numpy(), raw[:n * 5].view(n, 5)[:, 4].cpu().numpy(), enc[:n * 4].view(n, 4).cpu().numpy())


def _whole(P, generic, N):
    """A whole-array run of N samples drawn from the pool (tests/features_cases.whole_map) -> (outputs, sel)."""
    pl, sel = cases.pool(P), cases.whole_map(cases.pool(P)['D'], N)
    return _call(P, generic, pl['xyz'][sel], pl['knn'][sel]), sel


def _check_whole(P, generic, N, keep=None):
    out, sel = _whole(P, generic, N)
    if keep is not None:
        keep[N] = out
    name = f'P = {P}, N = {N}{", generic layout" if generic else ""}'
    return fr.check_features(name, cases.pool_truth(P, generic), 'eight', *out, sel=sel, form=_form(P, N))


def test_point_table_and_point_pack():
    """P = 1, 255, 256, 257 (one block, one block less a thread, two blocks with one live thread): table rows bit-equal to the
    restatement -- points beyond the bound give 32 zeros, the bound itself is in range, columns 32..34 are the learnable xyz,
    column 35 is 0, the 28 floats behind column 35 of a row are not written -- and the pack records bit-equal copies.
    MI355X: all bit-equal; 2 zero rows at P >= 255."""
    m = cases.model()
    for P in cases.P_TABLE:
        table, zeros = _point_table(P)
        sub = {k: v[:P] if isinstance(v, np.ndarray) and len(v) == 257 else v for k, v in m.items()}
        d = {'P': P, 'base': T(sub['base']), 'normals': T(sub['normals']), 'unit': T(sub['unit']), 'counter': T(sub['counter']), 'table': table.contiguous()}
        _point_pack(d, sub, table.cpu().numpy())
        print(f'   point_table / point_pack P = {P}: bit-equal, {zeros} zero rows')


def test_lanes8_whole_array_standard_layout():
    """sample_features8_kernel<false, *>: N through 1, 7, 8, 9, 31..33, 63..65, 95..97 and 6143 (256-thread blocks), 6144 and
    6145 (the LDS image) on the 257-point model; N = 6145 at P = 9216 (LDS image filled to its last record) and N = 97, 6145 at
    P = 9217 (one record too many: 256-thread blocks at any N).  Every check of features_restatement.check_features.
    MI355X: worst error / bound 0.043 of columns 0..34 over the 19 runs (P = 9216, N = 6145); everything else bit-equal."""
    worst = [_check_whole(257, False, N) for N in cases.N_LANES8]
    worst += [_check_whole(P, False, N) for P, N in ((cases.LDS_POINTS, 6145), (cases.LDS_POINTS + 1, 97), (cases.LDS_POINTS + 1, 6145))]
    print(f'8 lanes, standard layout: worst error / bound {max(worst):.3f} over {len(worst)} runs')


def test_lanes8_generic_layout():
    """sample_features8_kernel<true, *>: the same N with the last level cut to 12 344 entries (hashed, modulo); the columns of
    levels 0..14 bit-equal to the standard layout's run.
    MI355X: worst error / bound 0.042; levels 0..14 bit-equal in all 16 runs."""
    worst = []
    for N in cases.N_LANES8:
        got = {}
        worst.append(_check_whole(257, True, N, got))
        std = _whole(257, False, N)[0]
        ne = fr.bits(got[N][0][:, :66]) != fr.bits(std[0][:, :66])
        assert not ne.any(), f'N = {N}: column {np.argwhere(ne)[0][1]} of sample {np.argwhere(ne)[0][0]} depends on the last level\'s size'
        assert (fr.bits(got[N][0][:, 66:]) != fr.bits(std[0][:, 66:])).any() or N == 1
    print(f'8 lanes, generic layout: worst error / bound {max(worst):.3f} over {len(worst)} runs')


def _list_run(P, generic, rows, count, base, name):
    """A row list into the pool's own arrays against the whole-array run `base` of the pool, bit for bit; -> the worst error / bound."""
    pl = cases.pool(P)
    form = _form(P, len(rows))
    got = _call(P, generic, pl['xyz'], pl['knn'], rows=rows, count=count)
    sel = rows[:count].astype(np.int64)
    if count == 0:                                                                 # (nothing written: _call has seen every fill survive)
        return 0.0
    for what, g, b in zip(('mlp_in', 'distance', 'x'), got, base):
        ne = (fr.bits(g).reshape(count, -1) != fr.bits(b[sel]).reshape(count, -1))
        assert not ne.any(), (f'{name} ({form}): {what} of list entry {np.argwhere(ne)[0][0]} (sample {sel[np.argwhere(ne)[0][0]]}, slot '
                              f'{np.argwhere(ne)[0][0] & 7}) column {np.argwhere(ne)[0][1]} is not the whole-array run\'s')
    return fr.check_features(f'{name}, P = {P}', cases.pool_truth(P, generic), 'eight', *got, sel=sel, form=form)


def test_row_lists_with_device_count():
    """Ascending, unsorted with repeats, capacity beyond the count (the dead entries name a valid sentinel sample), count 1 and
    count 0, each in a tensor of 100 entries (256-thread blocks) and of 6 200 (the LDS image; at P = 9217 256-thread blocks
    again), standard and generic layout: bit-equal to the whole-array run on the listed samples, rows at and beyond the count
    untouched.
    MI355X: all 25 lists bit-equal; worst error / bound 0.042 of columns 0..34."""
    worst = []
    for P, generic, caps in ((257, False, (100, 6200)), (257, True, (100, 6200)), (cases.LDS_POINTS + 1, False, (6200,))):
        base = _call(P, generic, cases.pool(P)['xyz'], cases.pool(P)['knn'])
        for cap in caps:
            for name, rows, count in cases.row_lists(cases.pool(P)['D'], cap):
                worst.append(_list_run(P, generic, rows, count, base, f'{name}, capacity {cap}{", generic" if generic else ""}'))
    print(f'row lists: {len(worst)} lists bit-equal to the whole-array runs, worst error / bound {max(worst):.3f}')


@pytest.mark.parametrize('P,n', [(cases.LDS_POINTS, cases.LONG_LDS), (cases.LDS_POINTS + 1, cases.LONG_256)])
def test_row_lists_of_three_pipelined_trips(P, n):
    """49 157 entries over 256 x 96 sample groups (LDS image, P = 9216) and 524 293 over 8 192 x 32 (256-thread blocks,
    P = 9217): every group runs three trips of the software pipeline, the last one live for five entries only.  Compared on the
    device, by gather, with the whole-array run of the pool's 1 200 samples, which is itself held to the truth.
    MI355X: bit-equal in both forms; the pool's own run 0.043 (P = 9216) and 0.038 (P = 9217) of its bound."""
    pl = cases.pool(P)
    base = _call(P, False, pl['xyz'], pl['knn'], whole=True)
    D = pl['D']
    fr.check_features(f'the pool, P = {P}', cases.pool_truth(P), 'eight', base[0][:D * 68].view(D, 68).cpu().numpy(),
                      base[1][:D * 5].view(D, 5)[:, 4].cpu().numpy(), base[2][:D * 4].view(D, 4).cpu().numpy(), form=_form(P, D))
    rows = cases.long_list(D, n)
    groups = 256 * 96 if _form(P, n) == 'LDS form' else 8192 * 32
    assert -(-n // groups) == 3
    rows_d = T(rows)
    got = _call(P, False, pl['xyz'], pl['knn'], rows=rows_d, count=n, whole=True)
    idx = rows_d.long()
    for what, g, b, w, cols in (('mlp_in', got[0], base[0], 68, slice(0, 68)), ('distance', got[1], base[1], 5, slice(4, 5)), ('x', got[2], base[2], 4, slice(0, 4))):
        g2 = g[:n * w].view(n, w)[:, cols].view(torch.int32)
        b2 = b[:D * w].view(D, w)[:, cols].view(torch.int32)[idx]
        ne = g2 != b2
        if bool(ne.any()):
            o, c = (int(v) for v in ne.nonzero()[0])
            raise AssertionError(f'{_form(P, n)}, {n} entries: {what} of list entry {o} (sample {int(rows[o])}, slot {o & 7}, trip {o // groups}) '
                                 f'column {c} is not the whole-array run\'s')
    print(f'   {n} entries, {_form(P, n)}: three trips, bit-equal to the whole-array run by gather')


def test_encoder_range():
    """Rows 0..71 of the pool: trip t holds one sample whose x[0..2] > 1, at slot t, the ninth trip only such samples.  Their 32
    encoded columns are zero and every other sample of their trips has the restated bits -- on the 8-lanes kernel's two index
    paths (select and generic) and on the one-lane kernel.
    MI355X: 16 zero rows, 56 neighbours bit-equal, on all three."""
    pl = cases.pool()
    for generic, pack, name in ((False, True, '8 lanes, select'), (True, True, '8 lanes, generic'), (False, False, 'one lane')):
        tr = cases.pool_truth(257, generic)
        mlp_in, dist, x = _call(257, generic, pl['xyz'][:72], pl['knn'][:72], pack=pack)
        oob = np.zeros(72, bool)
        oob[pl['oob']] = True
        assert np.array_equal(((x < 0) | (x > 1)).any(1), oob) and not mlp_in[oob, 36:].any(), f'{name}: an out-of-range sample is not zero'
        ne = fr.bits(mlp_in[~oob, 36:]) != fr.bits(tr['enc'][:72][~oob])
        assert not ne.any() and mlp_in[~oob, 36:].any(1).all(), f'{name}: the trip neighbour {np.flatnonzero(~oob)[np.argwhere(ne)[0][0]]} of an out-of-range sample is wrong'
        print(f'   encoder range, {name}: {int(oob.sum())} zero rows, {int((~oob).sum())} neighbours bit-equal')


def test_one_lane_kernel():
    """sample_features_kernel: nscale 1..4 x (plain, att_in, geo_idxs, both) with N through 1, 255, 256, 257; att_in without a
    counter array; the host offsets NULL give the bits of the given ones.
    MI355X: worst error / bound 0.061 over the 16 cases (nscale 1: ten terms, rho_ref 0.25)."""
    m, lay = cases.model(), cases.layout()
    worst = []
    for c in cases.one_lane_cases():
        q = c['q']
        kw = dict(nscale=c['nscale'], geo_idxs=c['geo'], att_in=c['att_in'], pack=False, counter=c['att_in'] is None)
        got = _call(257, False, q['xyz'], q['knn'], **kw)
        worst.append(fr.check_features(c['name'], fr.truth(m, lay, q), 'one', *got, form='one lane'))
        null = _call(257, False, q['xyz'], q['knn'], h_given=False, **kw)
        assert all(np.array_equal(fr.bits(a), fr.bits(b)) for a, b in zip(got, null)), f'{c["name"]}: NULL host offsets change the bits'
    print(f'one lane: worst error / bound {max(worst):.3f} over {len(worst)} cases')


def test_one_lane_against_eight_lanes():
    """The pool through both kernels (4 scales, counts through the ids; the one-lane kernel is chosen by withholding the pack
    records): distance, x and the encoding bit-equal across them, columns 0..34 of each inside its own bound.
    MI355X: bit-equal; worst error / bound 0.037 (one lane) and 0.042 (8 lanes)."""
    pl, tr = cases.pool(), cases.pool_truth()
    one = _call(257, False, pl['xyz'], pl['knn'], pack=False)
    eight = _call(257, False, pl['xyz'], pl['knn'])
    for what, a, b in (('distance', one[1], eight[1]), ('x', one[2], eight[2]), ('encoding', one[0][:, 36:], eight[0][:, 36:])):
        assert np.array_equal(fr.bits(a), fr.bits(b)), f'{what} differs between the kernels'
    w1 = fr.check_features('the pool', tr, 'one', *one, form='one lane')
    w8 = fr.check_features('the pool', tr, 'eight', *eight, form=_form(257, pl['D']))
    print(f'cross-kernel: bit-equal in distance, x and encoding; worst error / bound {w1:.3f} / {w8:.3f}')


def test_centre_path_gives_the_plain_bits():
    """75 samples around a centre (tests/features_cases.centre_case): trips all inside the radius (copies of the centre: aggregate
    and encoding both copied; points beside it: aggregate copied, encoding computed), all outside, mixed (nothing copied), and a
    last trip of three live samples, all inside.  Every float of mlp_in, raw and enc_in equals the plain launch's.
    MI355X: bit-equal; 43 inside rows carry the centre's columns 0..35, 15 of them its x."""
    cc = cases.centre_case()
    pl = cases.pool()
    ci = cc['ci']
    c_mlp, c_dist, c_x = _call(257, False, pl['xyz'][ci:ci + 1], pl['knn'][ci:ci + 1])
    agg = T(np.concatenate([c_mlp[0, :36], c_x[0], c_mlp[0, 36:]]).astype(np.float32))
    center = T(np.concatenate([cc['c'], [cc['r2']]]).astype(np.float32))
    plain = _call(257, False, cc['xyz'], cc['knn'], whole=True)
    cached = _call(257, False, cc['xyz'], cc['knn'], center=center, center_agg=agg, whole=True)
    for name, a, b, w in (('mlp_in', plain[0], cached[0], 68), ('raw', plain[1], cached[1], 5), ('enc_in', plain[2], cached[2], 4)):
        ne = (a.view(torch.int32) != b.view(torch.int32)).cpu().numpy()
        assert not ne.any(), f'{name}: sample {np.flatnonzero(ne)[0] // w} (slot {(np.flatnonzero(ne)[0] // w) & 7}) column {np.flatnonzero(ne)[0] % w} differs from the plain launch'
    rows = plain[0][:75 * 68].view(75, 68).cpu().numpy()
    same = (fr.bits(rows[:, :36]) == fr.bits(c_mlp[0, :36])[None]).all(1)
    assert np.array_equal(same, cc['inside'])
    x = plain[2][:75 * 4].view(75, 4).cpu().numpy()
    same_x = (fr.bits(x) == fr.bits(c_x[0])[None]).all(1)
    assert same_x[cc['copy']].all() and (cc['inside'] & ~same_x).any(), 'both the copied and the computed encoding are met inside the radius'
    print(f'   centre path: bit-equal to the plain launch; {int(same.sum())} inside rows carry the centre\'s columns 0..35, {int(same_x.sum())} its x')
