"""GPU: composite_kernel (occnerf_amd/csrc/composite.hip), the forward compositor of the renderer and of the training step,
PER ENTRY against float64 train_path.raw2outputs of the fp32 inputs the launch read (tests/composite_forward_restatement.py:
the error weights, the tolerance 4 max(rho_ref, 1) measured on torch's fp32 CPU evaluation, the rule for term).

No norm over a tensor, no tolerance relative to the largest entry, no entry left out: rgb, acc, depth, every per-sample weight
and every term.  The C ABI writes into over-allocated buffers whose fill (256 bytes behind every output, and the rows out_rows
does not name) must survive.  Every launch is made three times -- all outputs, without weights and term, all outputs again -- and
what is requested must be bit-identical between them.  Each test prints what it saw; the values seen on an MI355X stand in
the docstrings."""
import numpy as np
import pytest
import torch

from tests import composite_forward_restatement as cf
from tests import step_backward_cases as cases
from tests.gpu_util import T, same

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FILL, IFILL, PAD = -7.5, -77, 64                          # 64 four-byte entries: 256 bytes behind every output


def _launch(c, want_w=True, want_term=True, out_rows=None, rows=None):
    """occnerf_composite on the case -> dict of numpy outputs (`rows` rows where out_rows scatters; n otherwise), after the
    fill behind every buffer has been seen to survive."""
    from occnerf_amd import _lib, ops
    n, S = c['z'].shape
    rows = n if rows is None else rows
    raw, mask, z, rays = T(c['raw']), T(c['mask']), T(c['z']), T(c['rays8'])
    rgb = torch.full((rows * 3 + PAD,), FILL, device=DEV)
    acc = torch.full((rows + PAD,), FILL, device=DEV)
    dep = torch.full((rows + PAD,), FILL, device=DEV)
    w = torch.full((n * S + PAD,), FILL, device=DEV) if want_w else None
    tp = torch.full((rows + PAD,), IFILL, device=DEV, dtype=torch.int32) if want_term else None
    orows = None if out_rows is None else torch.from_numpy(np.ascontiguousarray(out_rows, np.int64)).to(DEV)
    _keep, pbg = ops._host_f32(c['bg'], 3)
    with ops._guard(raw):
        rc = _lib.lib().occnerf_composite(raw.data_ptr(), mask.data_ptr(), z.data_ptr(), rays.data_ptr(), pbg, n, S, rgb.data_ptr(),
                                          acc.data_ptr(), dep.data_ptr(), None if w is None else w.data_ptr(),
                                          None if tp is None else tp.data_ptr(), None if orows is None else orows.data_ptr(),
                                          ops._stream(raw))
    _lib.check(rc, 'composite')
    torch.cuda.synchronize()
    out = {'rgb': (rgb, rows * 3), 'acc': (acc, rows), 'depth': (dep, rows), 'w': (w, n * S), 'term': (tp, rows)}
    res = {}
    for k, (t, size) in out.items():
        if t is None:
            res[k] = None
            continue
        a = t.cpu().numpy()
        assert np.all(a[size:] == (IFILL if k == 'term' else FILL)), f'composite: the fill behind {k} must survive'
        res[k] = a[:size]
    res['rgb'] = res['rgb'].reshape(rows, 3)
    if want_w:
        res['w'] = res['w'].reshape(n, S)
    return res


def _three_launches(name, c):
    """All outputs; without weights and term; all outputs again: what is requested is bit-identical."""
    full = _launch(c)
    bare = _launch(c, want_w=False, want_term=False)
    again = _launch(c)
    assert bare['w'] is None and bare['term'] is None
    for k in ('rgb', 'acc', 'depth'):
        same(bare[k].view(np.uint32), full[k].view(np.uint32), f'{name}: {k} without weights / term')
    for k in ('rgb', 'acc', 'depth', 'w'):
        same(again[k].view(np.uint32), full[k].view(np.uint32), f'{name}: {k} of a second call')
    same(again['term'], full['term'], f'{name}: term of a second call')
    only_w, only_t = _launch(c, want_term=False), _launch(c, want_w=False)
    same(only_w['w'].view(np.uint32), full['w'].view(np.uint32), f'{name}: weights without term')
    same(only_t['term'], full['term'], f'{name}: term without weights')
    for o in (only_w, only_t):
        for k in ('rgb', 'acc', 'depth'):
            same(o[k].view(np.uint32), full[k].view(np.uint32), f'{name}: {k} with one optional output')
    return full


@pytest.mark.parametrize('bg', [0, 1])
@pytest.mark.parametrize('S', cases.COMPOSITE_S)
def test_composite_forward_per_entry(S, bg):
    """41 rays: x = 25 / 20 / 20 + ulp / -30, mask 0 (every weight exactly 0, term 0), alpha = 1 exactly (tt = fl(1e-10)),
    alpha > 1 (tt < 0), equal consecutive z, direction norms 1e-3 and 1e3, 29 random rays; both backgrounds; S on both sides of
    every 64-sample chunk boundary of the scan, and S = 1.
    MI355X, rho_ref / kernel on the random rows at S = 1, 2, 63, 64, 65, 128, 129, 192, 256: 0.17/0.17, 0.77/0.58, 0.50/0.68,
    0.50/0.60, 0.69/0.69, 0.51/0.61, 0.53/0.62, 0.50/0.60, 0.50/0.62 (the same for both backgrounds); every special kind at most
    0.53 on the reference's side and 0.64 on the kernel's (norm 1e-3 at S = 256), against a tolerance of 4; the mask = 0 ray's
    weights exactly 0; no random ray's term undecided."""
    c = cases.composite_case(S, cases.BACKGROUNDS[bg])
    cf.check_forward(f'S={S} bg={bg}', c, _three_launches(f'S={S} bg={bg}', c))


@pytest.mark.parametrize('S', [1, 64])
def test_composite_forward_one_ray(S):
    """n = 1: one block, three idle waves.  MI355X: rho_ref / kernel 0.09/0.09 at S = 1, 0.48/0.48 at S = 64."""
    c = cases.composite_plain(1, S, 1)
    cf.check_forward(f'n=1 S={S}', c, _three_launches(f'n=1 S={S}', c))


def test_composite_forward_grid_stride():
    """n = 32 768 + 5 rays of 2 samples: the launch caps at 8 192 blocks of 4 waves, so rays 32 768.. are the second trip of the
    grid-stride loop, reported as their own group.
    MI355X: rho_ref / kernel 0.91/0.95 on the first trip, 0.52/0.52 on the second; no term undecided among 32 773."""
    c = cases.composite_plain(32768 + 5, 2, 2)
    got = _three_launches('n=32773 S=2', c)
    c['groups'] = {'random': np.arange(32768), 'second trip': np.arange(32768, 32768 + 5)}
    cf.check_forward('n=32773 S=2', c, got)


@pytest.mark.parametrize('S', [257, 300])
def test_composite_forward_more_than_256_samples(S):
    """The forward takes any S (only the backward refuses): five chunks of the scan, the last of 1 and of 44 samples.
    MI355X: rho_ref / kernel 0.50/0.62 at S = 257, 0.48/0.62 at S = 300."""
    c = cases.composite_plain(9, S, 3)
    cf.check_forward(f'S={S}', c, _three_launches(f'S={S}', c))


def test_composite_forward_out_rows():
    """out_rows: a permutation of 41 rays into buffers of 41 + 7 rows; row out_rows[r] is bit-identical to row r of the plain
    launch and the 7 rows nobody names keep their fill.
    MI355X: every named row bit-identical, the 7 others untouched; ratios those of S = 65."""
    c = cases.composite_case(65)
    n = c['z'].shape[0]
    rows = n + 7
    perm = np.random.RandomState(5).permutation(rows)[:n]
    plain = _launch(c)
    got = _launch(c, out_rows=perm, rows=rows)
    for k in ('rgb', 'acc', 'depth', 'term'):
        same(got[k][perm], plain[k], f'out_rows: {k}')
        rest = np.delete(got[k], perm, axis=0)
        assert len(rest) == 7 and np.all(rest == (IFILL if k == 'term' else FILL)), f'out_rows: the unnamed rows of {k} keep their fill'
    same(got['w'].view(np.uint32), plain['w'].view(np.uint32), 'out_rows: weights stay in ray order')
    cf.check_forward('out_rows S=65', c, {k: (got[k][perm] if k != 'w' else got[k]) for k in got})
    print(f'out_rows: {n} rays into {rows} rows, 7 rows untouched')
