"""CPU: occnerf_amd/packed.py, the one place that picks the MLP kernel for a cfg.mlp_precision.  The ops functions are replaced
by recorders ON THE ops MODULE (as bench.py, tests and tools replace them), with the signatures bench.py's timing wrappers have:
a call form those wrappers could not bind, or a function bound before the replacement, fails here."""
import types

import pytest
import torch
import torch.nn as nn

from occnerf_amd import ops, packed

PACKS = ('canonical_mlp_pack', 'canonical_mlp_pack_bf16', 'canonical_mlp_pack_f16',
         'nonrigid_pack', 'nonrigid_pack_bf16', 'nonrigid_pack_f16')
PACK_DTYPE = {'canonical_mlp_pack_bf16': torch.bfloat16, 'nonrigid_pack_bf16': torch.bfloat16,
              'canonical_mlp_pack_f16': torch.float16, 'nonrigid_pack_f16': torch.float16}
SPLIT_DTYPE = {'fp32': None, 'bf16x3': torch.bfloat16, 'f16x3': torch.float16}


@pytest.fixture
def calls(monkeypatch):
    """[(ops function name, positional arguments, keyword arguments)] of everything the object under test reaches."""
    log = []

    def pack(name):
        def fn(*a, **k):
            log.append((name, a, k))
            return torch.zeros(4, dtype=PACK_DTYPE.get(name, torch.float32))
        return fn
    for name in PACKS:
        monkeypatch.setattr(ops, name, pack(name))

    def canonical_mlp(mlp_in, packed, raw, count=None, **kw):                       # bench.py: timed_mlp
        log.append(('canonical_mlp', (mlp_in, packed, raw), dict(kw, count=count)))
        return raw

    def nonrigid_rows(xyz, rows, count, *a, **kw):                                  # bench.py: timed_nr
        log.append(('nonrigid_rows', (xyz, rows, count) + a, kw))
        return xyz

    def other(name):
        def fn(*a, **k):                                                            # bench.py: timed_mlp2
            log.append((name, a, k))
            return a[0]
        return fn
    monkeypatch.setattr(ops, 'canonical_mlp', canonical_mlp)
    monkeypatch.setattr(ops, 'nonrigid_rows', nonrigid_rows)
    for name in ('canonical_mlp_bf16x3', 'nonrigid', 'nonrigid_bf16x3', 'nonrigid_bf16x3_rows'):
        monkeypatch.setattr(ops, name, other(name))
    return log


def _modules():
    torch.manual_seed(0)
    lins = [nn.Linear(8, 8) for _ in range(3)]
    cnl = types.SimpleNamespace(linear_params=lambda: ([m.weight for m in lins], [m.bias for m in lins]))
    nr = types.SimpleNamespace(block_mlps=[nn.Linear(8, 8), nn.ReLU(), nn.Linear(8, 8), nn.ReLU(), nn.Linear(8, 3)])
    return cnl, nr


def _names(log):
    return [c[0] for c in log]


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'f16x3'])
def test_packs_in_order(calls, precision):
    pk = packed.PackedMLPs(*_modules(), precision, True)
    tail = {'fp32': '', 'bf16x3': '_bf16', 'f16x3': '_f16'}[precision]
    want = ['canonical_mlp_pack'] + (['canonical_mlp_pack' + tail] if tail else []) + \
           ['nonrigid_pack'] + (['nonrigid_pack' + tail] if tail else [])
    assert _names(calls) == want
    for split in (pk.cnl_split, pk.nr_split):
        assert (split is None) if tail == '' else (split.dtype == SPLIT_DTYPE[precision])
    assert (pk.domain_flag is not None) == (precision == 'f16x3')
    if pk.domain_flag is not None:
        assert pk.domain_flag.dtype == torch.int32 and int(pk.domain_flag) == 0


@pytest.mark.parametrize('check', [True, 'deferred', False])
def test_domain_flag_follows_the_check_mode(calls, check):
    assert (packed.PackedMLPs(*_modules(), 'f16x3', check).domain_flag is not None) == bool(check)


@pytest.mark.parametrize('listed', [False, True], ids=['whole', 'rows'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'f16x3'])
def test_offsets_and_canonical_reach_the_parent_s_function(calls, precision, listed):
    pk = packed.PackedMLPs(*_modules(), precision, True)
    del calls[:]
    xyz, cond, hann = torch.zeros(6, 3), torch.zeros(69), [1.0] * 6
    rows, count = (torch.arange(6, dtype=torch.int32), torch.tensor([4], dtype=torch.int32)) if listed else (None, None)
    split = precision != 'fp32'

    pk.offsets(xyz, cond, hann, rows=rows, count=count, out=xyz)
    (name, a, k), = calls
    assert name == {(False, False): 'nonrigid', (False, True): 'nonrigid_rows',
                    (True, False): 'nonrigid_bf16x3', (True, True): 'nonrigid_bf16x3_rows'}[(split, listed)]
    lead = (xyz, rows, count) if listed else (xyz,)
    weights = (pk.nr_w0, pk.nr_b0, pk.nr) + ((pk.nr_split,) if split else ())
    assert len(a) == len(lead) + 2 + len(weights)
    assert all(x is y for x, y in zip(a, lead + (cond, hann) + weights))
    want_kw = {} if listed else {'out': xyz}
    if split:
        want_kw['domain_flag'] = pk.domain_flag
    assert set(k) == set(want_kw) and all(k[n] is want_kw[n] for n in k)

    del calls[:]
    mlp_in, raw = torch.zeros(7, 68), torch.zeros(6, 5)
    in_rows = rows
    pk.canonical(mlp_in, raw, count=count, in_rows=in_rows)
    (name, a, k), = calls
    assert name == ('canonical_mlp_bf16x3' if split else 'canonical_mlp')
    want_a = (mlp_in, pk.cnl, pk.cnl_split, raw) if split else (mlp_in, pk.cnl, raw)
    assert len(a) == len(want_a) and all(x is y for x, y in zip(a, want_a))
    assert k.pop('count') is count and k.pop('in_rows') is in_rows
    assert (k.pop('domain_flag') is pk.domain_flag) if split else True
    assert not k


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'f16x3'])
def test_exact_shares_the_packs_and_packs_nothing(calls, precision):
    pk = packed.PackedMLPs(*_modules(), precision, True)
    n_packs = len(calls)
    ex = pk.exact()
    assert len(calls) == n_packs
    assert ex.cnl is pk.cnl and ex.nr is pk.nr and ex.nr_w0 is pk.nr_w0 and ex.nr_b0 is pk.nr_b0 and ex.key == pk.key
    assert ex.cnl_split is None and ex.nr_split is None and ex.domain_flag is None
    assert (pk.nr_split is None) == (precision == 'fp32'), 'the object itself is left as it was'
    xyz, rows, count = torch.zeros(6, 3), torch.arange(6, dtype=torch.int32), torch.tensor([6], dtype=torch.int32)
    ex.offsets(xyz, torch.zeros(69), [1.0] * 6, out=xyz)
    ex.offsets(xyz, torch.zeros(69), [1.0] * 6, rows=rows, count=count)
    ex.canonical(torch.zeros(6, 68), torch.zeros(6, 5), count=count)
    assert _names(calls[n_packs:]) == ['nonrigid', 'nonrigid_rows', 'canonical_mlp']


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'f16x3'])
def test_training_stream_is_split_fp16_and_packed_once(calls, precision):
    pk = packed.PackedMLPs(*_modules(), precision, True)
    n_packs = len(calls)
    word = torch.zeros(1, dtype=torch.int32)
    views = [pk.train_f16x3(word), pk.train_f16x3(None)]
    assert _names(calls[n_packs:]) == ([] if precision == 'f16x3' else ['nonrigid_pack_f16'])
    assert views[0].nr_split is views[1].nr_split and views[0].nr_split.dtype == torch.float16
    assert views[0].domain_flag is word and views[1].domain_flag is None and views[0].nr is pk.nr
    if precision == 'f16x3':
        assert views[0].nr_split is pk.nr_split
    del calls[:]
    views[0].offsets(torch.zeros(6, 3), torch.zeros(69), [1.0] * 6)
    (name, a, k), = calls
    assert name == 'nonrigid_bf16x3' and a[-1] is views[0].nr_split and k['domain_flag'] is word and k['out'] is None


def test_cache_key(calls):
    cnl, nr = _modules()
    key = packed.PackedMLPs.cache_key(cnl, nr, 'fp32', True)
    assert key == packed.PackedMLPs.cache_key(cnl, nr, 'fp32', True)
    assert key != packed.PackedMLPs.cache_key(cnl, nr, 'f16x3', True)
    assert key != packed.PackedMLPs.cache_key(cnl, nr, 'fp32', 'deferred')
    with torch.no_grad():
        nr.block_mlps[2].bias.add_(1.0)                 # an optimizer step: in place, the version counter moves
    assert key != packed.PackedMLPs.cache_key(cnl, nr, 'fp32', True)
    with pytest.raises(RuntimeError, match='mlp_precision'):
        packed.PackedMLPs.cache_key(cnl, nr, 'fp16', True)
    assert not calls, 'asking for the key packs nothing'
    assert packed.PackedMLPs(cnl, nr, 'bf16x3', False).key == packed.PackedMLPs.cache_key(cnl, nr, 'bf16x3', False)
