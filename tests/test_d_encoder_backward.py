"""GPU: every route of the D = 4, C = 2 hash encoder's backward (occnerf_amd/csrc/grid_encode.hip) against the float64
restatement of tests/encoder_backward_restatement.py, per table cell and with the derived budgets written there -- no
tolerance relative to the largest entry, under which a kernel that dropped every small cell would pass.

Routes, each on the same input and each with its own bound (u = 2^-24, A = sum of |terms| of the cell, n its term count):
    op        ops.grid_encode_backward: tiled kernel + tile-set masks from 32 768 samples up     gamma_{nsl+1} A + n 2^-53 A
    op_plain  occnerf_grid_encode_backward_h without scratch: tiled kernel, plain scan           the same
    scatter   occnerf_grid_encode_backward (no host offsets): always the scatter kernel          gamma_{n-1} A
    module    GridEncoder(...)(x).backward(g): runs merged from 4 096 up, then `op`              op's bound + gamma_66 A
    module_gi the same with x.requires_grad_(): no merge, `op` + the input-gradient kernel        op's bound; gi bit-equal
Below 32 768 samples, and from 65 536 tile-jobs up, `op` and `op_plain` are the scatter kernel and get its bound.  Cells
with one term must be bit-equal to fp32(w * g) on every route, cells without terms exactly zero.

Each test prints its worst error / bound per route; the values measured on an MI355X stand in the docstrings."""
import numpy as np
import pytest
import torch

from tests import encoder_backward_cases as cases
from tests import encoder_backward_restatement as ebr
from tests.gpu_util import DEV, T, same

pytestmark = pytest.mark.gpu

D, C = 4, 2
TILED_FROM = 32768                          # grid_backward_impl: B >= 32768 with host offsets takes the tiled kernel
MAX_TILE_JOBS = 65536                       # ... while the launch stays below this many tile-jobs


def _in_range(x):
    return ~((x < 0) | (x > 1)).any(1)


def _to_levels(rows, L):
    """autograd's [B, L*C] rows -> the operator's [L, B, C]."""
    return np.ascontiguousarray(rows.reshape(len(rows), L, C).transpose(1, 0, 2))


class _Case:
    """One (layout, input, gradient): the reference, computed once, and the comparison of a device table against it."""

    def __init__(self, layout, x, rows, sparse):
        self.layout, self.spec = layout, cases.LAYOUTS[layout]
        self.off, self.S, self.H = cases.layout_offsets(layout)
        self.L, self.total, self.B = len(self.off) - 1, int(self.off[-1]), len(x)
        self.x, self.rows, self.gl = x, rows, _to_levels(rows, self.L)
        self.modes, self.tiles, self.slices, self.jobs = cases.tile_jobs(self.off, self.S, self.H)
        self.tiled = self.B >= TILED_FROM and self.jobs < MAX_TILE_JOBS
        if sparse:
            self.idx, self.ssum, self.A, self.n = ebr.backward_numpy_sparse(self.gl, x, self.off, C, self.S, self.H)
        else:
            self.idx = None
            self.ssum, self.A, self.n = ebr.backward_numpy(self.gl, x, self.off, C, self.S, self.H)
        assert int(self.n.sum()) == int(_in_range(x).sum()) * 16 * self.L
        self.nsl = cases.slices_per_entry(self.off, self.S, self.H, self.idx)
        self.offsets = T(self.off)
        self.xt, self.glt = T(x), T(self.gl)
        self.worst = {}

    def bound(self, route):
        tiled = ebr.bound_tiled(self.A, self.n, self.nsl) if self.tiled else ebr.bound_serial(self.A, self.n)
        return {'op': tiled, 'op_plain': tiled, 'module_gi': tiled, 'scatter': ebr.bound_serial(self.A, self.n),
                'module': tiled + ebr.bound_runs(self.A)}[route]

    def check(self, route, table):
        torch.cuda.synchronize()
        if self.idx is None:
            got = table.cpu().numpy()
        else:                                                   # sparse: the touched entries, and an exact zero everywhere else
            pick = torch.from_numpy(self.idx).to(DEV)
            got = table[pick].cpu().numpy()
            table[pick] = 0.0
            assert int(torch.count_nonzero(table)) == 0, f'{route}: entries no sample touches are not zero'
        self.worst[route] = ebr.check(f'{self.layout} B={self.B} {route}', got, self.ssum, self.bound(route), self.n)

    def zeros(self):
        return torch.zeros(self.total, C, device=DEV)

    def run_op(self, ops):
        out = self.zeros()
        ops.grid_encode_backward(self.glt, self.xt, out, self.offsets, out, self.B, D, C, self.L, self.S, self.H)
        self.check('op', out)

    def run_raw(self, ops, host_offsets):
        from occnerf_amd import _lib
        out = self.zeros()
        stream = torch.cuda.current_stream().cuda_stream
        head = [self.glt.data_ptr(), self.xt.data_ptr(), out.data_ptr(), self.offsets.data_ptr()]
        tail = [out.data_ptr(), self.B, D, C, self.L, self.S, self.H, None, None, 0, 0, 0]
        if host_offsets:                                        # no scratch: the tiled kernel's plain scan
            rc = _lib.lib().occnerf_grid_encode_backward_h(*head, ops._host_offsets(self.offsets), *tail, None, 0, stream)
        else:                                                   # no host offsets: the scatter kernel
            rc = _lib.lib().occnerf_grid_encode_backward(*head, *tail, stream)
        _lib.check(rc, 'grid_encode_backward')
        self.check('op_plain' if host_offsets else 'scatter', out)

    def encoder(self):
        """-> (x -> [B, L*C] through the module, its embeddings parameter).  Level sizes the constructor never produces go
        through the module's autograd Function on the layout's own offsets."""
        from occnerf_amd.gridencoder import GridEncoder, grid_encode
        if 'resize' in self.spec:
            pls = cases.layout_offsets(self.layout, with_scale=True)[3]
            emb = torch.nn.Parameter(torch.empty(self.total, C, device=DEV).uniform_(-1, 1))
            return (lambda x: grid_encode(x, emb, self.offsets, pls, self.H, x.requires_grad, 0, False, 0)), emb
        enc = GridEncoder(input_dim=D, num_levels=self.L, level_dim=C, per_level_scale=2.0, base_resolution=self.H,
                          log2_hashmap_size=self.spec['log2'], desired_resolution=self.spec['desired']).to(DEV)
        assert np.array_equal(enc.offsets.cpu().numpy(), self.off) and abs(enc.log2_per_level_scale - self.S) < 1e-12
        with torch.no_grad():
            enc.embeddings.uniform_(-1, 1)
        return (lambda x: enc(x, bound=None)), enc.embeddings

    def run_module(self):
        encode, emb = self.encoder()
        encode(self.xt).backward(T(self.rows))
        self.check('module', emb.grad)

    def run_module_input_grad(self, oracle):
        """The input gradient is a fixed-order fp32 chain over (level, channel): bit-equal to the oracle's, which
        tests/test_encoder_backward_restatement.py pins to the same chain in numpy."""
        encode, emb = self.encoder()
        xg = self.xt.clone().requires_grad_()
        encode(xg).backward(T(self.rows))
        _, dy = oracle.grid_encode_forward(self.x, emb.detach().cpu().numpy(), self.off, self.S, self.H, True)
        _, want = oracle.grid_encode_backward(self.gl, self.x, self.off, self.total, C, self.S, self.H, dy)
        assert np.array_equal(want.view(np.uint32), ebr.input_grad_chain32(self.gl, dy, D).view(np.uint32))
        same(xg.grad.cpu().numpy().view(np.uint32), want.view(np.uint32), 'input gradient')
        assert not xg.grad[~torch.from_numpy(_in_range(self.x)).to(DEV)].any()
        self.check('module_gi', emb.grad)

    def run_all(self, ops, oracle):
        self.run_op(ops)
        self.run_raw(ops, host_offsets=True)
        self.run_raw(ops, host_offsets=False)
        self.run_module()
        self.run_module_input_grad(oracle)
        return self.worst


def _inputs(kind, B, L, seed):
    """-> (x [B, 4], grad rows [B, L*C]); asserts inside the callers keep every one of them from being degenerate."""
    x = cases.training_like_inputs(B, seed)
    rows = cases.training_like_grads(L, B, C, seed)
    rng = np.random.default_rng(seed + 77)
    if kind == 'uniform':
        x = rng.random((B, D), dtype=np.float32)
    elif kind == 'hot':                                         # one hot cell: every row the same in-range point
        x[:] = np.array([0.673, 0.412, 0.0203, 0.31], np.float32)
    elif kind == 'oob':                                         # every row out of range, on one axis or another
        x[np.arange(B), np.arange(B) % D] = np.where(np.arange(B) % 3 == 0, -0.125, 1.0 + 2.0 ** -20).astype(np.float32)
    elif kind == 'zero_grad':
        rows[:] = 0.0
        rows[1::2] = -0.0
    else:
        assert kind == 'training'
    return x, rows


@pytest.mark.parametrize('kind,B', [('uniform', 40000), ('training', 32767), ('training', 32768), ('training', 32769),
                                    ('training', 33280), ('training', 40000), ('hot', 32768), ('oob', 32768), ('zero_grad', 32768)])
def test_backward_routes_default_layout(ops, oracle, kind, B):
    """The training step's table (2 dense + 14 hashed 2^19 levels, 8 000 tile-jobs) around the 32 768 threshold: 32 767 is the
    scatter kernel on every route, 32 769 leaves sample slices 13-15 of the dense levels empty, 33 280 = 65 x 512 ends on a
    wave-chunk boundary.  Inputs: uniform; training-like (half the rows in one cluster, runs of identical rows, edges, ~1 %
    out of range; gradient rows with exactly one zero channel, which must contribute); one hot cell (B terms on each of its 16
    corners per level: the same-address LDS atomic); all rows out of range and all gradients zero (the table stays exactly 0).
    Measured on an MI355X, worst error / bound: tiled routes (op, op_plain, module_gi) 0.26-0.38 on the uniform and the
    training-like inputs at every batch size, 0.003 on the hot cell; module (runs of 2 ... 5 000 rows merged) 0.03-0.05; scatter 1.000 (cells of
    two terms, whose one rounding can use the whole of gamma_1 A) -- at 32 767 every route but `module` is the scatter
    kernel and shows 1.000; out-of-range and zero-gradient inputs: 0, every table exactly zero."""
    x, rows = _inputs(kind, B, 16, seed=B % 1000 + len(kind))
    case = _Case('default', x, rows, sparse=False)
    assert case.modes == 'DD' + 'P' * 14 and case.jobs == 8000 and case.tiled == (B >= 32768)
    inr = _in_range(x)
    if kind == 'uniform':
        assert inr.all() and case.n.max() >= 16
    elif kind == 'hot':
        assert inr.all() and case.n.max() >= B
    elif kind == 'oob':
        assert not inr.any() and case.n.max() == 0
    else:
        assert inr.sum() >= 0.97 * B and inr[:B // 2].sum() >= 0.97 * (B // 2) and not inr.all()
        assert case.n.max() >= B // 4                           # the cluster's cell on the coarse levels
        assert set(cases.RUN_LENGTHS) <= set(cases.run_lengths(x).tolist())     # the runs are whole
    if kind == 'zero_grad':
        assert not case.A.any()
    elif kind != 'oob':
        g3 = rows.reshape(B, 16, C)
        one_zero = ((g3[..., 0] == 0) != (g3[..., 1] == 0)).any(1) & inr
        assert one_zero.sum() >= B // 5                         # rows (0, g) / (g, 0): they contribute
    worst = case.run_all(ops, oracle)
    assert set(worst) == {'op', 'op_plain', 'scatter', 'module', 'module_gi'}
    if kind in ('oob', 'zero_grad'):
        assert max(worst.values()) == 0.0


@pytest.mark.parametrize('layout', ['generic', 'log2_20', 'log2_14', 'L1', 'L2', 'L5'])
def test_backward_routes_other_layouts(ops, oracle, layout):
    """Level layouts that reach the other branches of the tiled dispatch, at 32 769 training-like samples: hashed levels whose
    size is no power of two (generic index in the mask pre-pass and in the tile scan, partial last tile); 128 tiles per level
    (masks dropped although scratch is passed); two tiles per level (8 slices each, heavy merging); 1, 2 and 5 levels (the
    first_block walk and the l >= L guards; the module route then merges runs with the general kernel).  Modes and tile-jobs
    are asserted through the host's own arithmetic (tests/test_encoder_backward_restatement.py holds the whole table).
    Measured on an MI355X, worst error / bound: op and op_plain 0.30 (generic, 2^20), 0.39 (2^14), 0.14 / 0.29 / 0.35
    (L = 1 / 2 / 5); module (all seven runs whole) 0.03-0.05; scatter 0.99-1.00."""
    B = 32769
    L = cases.LAYOUTS[layout]['L']
    x, rows = _inputs('training', B, L, seed=len(layout) + L)
    case = _Case(layout, x, rows, sparse=True)
    want = {'generic': ('DDPGPPGPPPPPPPPG', 7384), 'log2_20': ('DD' + 'P' * 14, 15168), 'log2_14': ('P' * 16, 256),
            'L1': ('D', 176), 'L2': ('DP', 688), 'L5': ('DPPPP', 2224)}[layout]
    assert (case.modes, case.jobs) == want and case.tiled
    if layout == 'log2_20':
        assert max(case.tiles) == 128
    if layout == 'generic':
        assert [case.tiles[l] for l in (3, 6, 15)] == [37, 16, 62]
    assert _in_range(x).sum() >= 0.97 * B and case.n.max() >= B // 4
    assert set(cases.RUN_LENGTHS) <= set(cases.run_lengths(x).tolist())
    case.run_all(ops, oracle)


@pytest.mark.parametrize('layout', ['big_L15', 'big_L16'])
def test_backward_largest_tiled_launch_and_its_fallback(ops, oracle, layout):
    """Base resolution 64, 2^22 entries per level (512 tiles, all hashed; 0.5 GB of fp32 on the device): 15 levels are 61 440
    tile-jobs, the largest launch the tiled kernel takes (unmasked: more than 64 tiles); 16 levels are 65 536 and fall back to
    the scatter kernel, whose bound then applies.  Sparse restatement; entries no sample touches are checked for exact zeros
    on the device.
    Measured on an MI355X, worst error / bound: 15 levels (tiled) 0.254 on both routes, 16 levels (scatter) 1.000."""
    B = 32768
    L = cases.LAYOUTS[layout]['L']
    x, rows = _inputs('training', B, L, seed=L)
    case = _Case(layout, x, rows, sparse=True)
    assert case.modes == 'P' * L and case.tiles == [512] * L and case.jobs == 4096 * L
    assert case.tiled == (layout == 'big_L15')
    assert _in_range(x).sum() >= 0.97 * B and case.n.max() >= B // 5
    case.run_op(ops)
    case.run_raw(ops, host_offsets=True)


def test_backward_training_batch(ops, oracle):
    """The training step's own batch, 6 144 rays x 128 samples = 786 432 training-like encoder inputs, through the operator
    (tiled + masks) and through the module (runs merged first): the fullest cell collects over 200 000 terms.
    Measured on an MI355X, worst error / bound: op 0.442, module 0.050 (fullest cell 220 072 terms); 10 s with the
    reference."""
    B = 786432
    x, rows = _inputs('training', B, 16, seed=1)
    case = _Case('default', x, rows, sparse=False)
    assert case.tiled and _in_range(x).sum() >= 0.97 * B and case.n.max() >= B // 4
    assert set(cases.RUN_LENGTHS) <= set(cases.run_lengths(x).tolist())
    case.run_op(ops)
    case.run_module()


@pytest.mark.parametrize('layout', ['generic', 'log2_20', 'log2_14'])
@pytest.mark.parametrize('B', [32767, 32769])
def test_forward_index_modes_of_the_operator(ops, oracle, layout, B):
    """The operator's D = 4, C = 2 forward -- sample-major below 32 768 samples, levels dealt to the XCDs from there up -- on
    the layouts whose generic index mode only the fused feature kernel's copy reached: bit-equal to the oracle."""
    off, S, H = cases.layout_offsets(layout)
    L = len(off) - 1
    x = cases.training_like_inputs(B, 3)
    emb = np.random.default_rng(B).uniform(-1, 1, (int(off[-1]), C)).astype(np.float32)
    out = torch.empty(L, B, C, device=DEV)
    ops.grid_encode_forward(T(x), T(emb), T(off), out, B, D, C, L, S, H)
    want, _ = oracle.grid_encode_forward(x, emb, off, S, H)
    same(out.cpu().numpy().view(np.uint32), want.view(np.uint32), f'forward {layout} B={B}')
    assert want[:, _in_range(x)].any() and not want[:, ~_in_range(x)].any()


def test_backward_float64_dispatch_training_like(ops):
    """scalar_t = double (`_f64` entry: double atomics in any order) at 40 000 training-like samples.  Term: double(w) * g,
    rounded once, w the fp32 corner weight; reference sum in extended precision; bound n 2^-53 A per cell, single-term cells
    equal, untouched entries exactly zero.
    Measured on an MI355X, worst error / bound: 0.948 (fullest cell 11 234 terms)."""
    B, L = 40000, 16
    off, S, H = cases.layout_offsets('default')
    x = cases.training_like_inputs(B, 64)
    gl = _to_levels(cases.training_like_grads(L, B, C, 64), L).astype(np.float64)
    gl *= np.random.default_rng(64).uniform(1.0, 1.0 + 2.0 ** -30, gl.shape)            # (not fp32-representable)
    idx, ssum, A, n = ebr.backward_numpy_sparse(gl, x, off, C, S, H, f64_terms=True)
    assert _in_range(x).sum() >= 0.97 * B and n.max() >= B // 4
    out = torch.zeros(int(off[-1]), C, device=DEV, dtype=torch.float64)
    ops.grid_encode_backward(T(gl), T(x), out, T(off), out, B, D, C, L, S, H)
    pick = torch.from_numpy(idx).to(DEV)
    got = out[pick].cpu().numpy()
    out[pick] = 0.0
    assert int(torch.count_nonzero(out)) == 0
    ebr.check('float64 dispatch', got, ssum, ebr.bound_f64(A, n), n, bit_equal_single=False)
    assert np.array_equal(got[n == 1], ssum[n == 1])
