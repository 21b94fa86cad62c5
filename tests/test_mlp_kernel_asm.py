"""CPU: what the compiler makes of the streamed MLP kernels -- the two fp32 LDS-staged ones (mlp16.hip, nonrigid16.hip), the
split-operand kernels (mlp.hip, nonrigid.hip) and the fused trunk forward (trunks.hip), all on the ring of weight_ring.h.

Beside an fp32 MFMA nothing else issues on a gfx950 SIMD, so the kernels' budget of other instructions and their
register / LDS footprint (two waves per SIMD, two workgroups per CU) are part of what they are.  Each source is
cross-compiled ONCE to assembly with the Makefile's own flags; no GPU is needed.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'occnerf_amd', 'csrc')


def _makefile_var(name):
    text = open(os.path.join(CSRC, 'Makefile')).read()
    m = re.search(r'^%s\s*\?=\s*(.*)$' % name, text, re.M)
    assert m, name
    return m.group(1).strip()


def _hipcc():
    for cand in (os.environ.get('HIPCC'), _makefile_var('HIPCC'), shutil.which('hipcc')):
        if cand and os.path.exists(cand):
            return cand
    return None


pytestmark = pytest.mark.skipif(_hipcc() is None, reason='hipcc is not installed')


def _compile(src, outdir):
    flags = _makefile_var('FLAGS').replace('$(ARCH)', _makefile_var('ARCH')).split()
    out = os.path.join(str(outdir), src.replace('.hip', '.s'))
    subprocess.run([_hipcc()] + flags + ['--cuda-device-only', '-S', os.path.join(CSRC, src), '-o', out], check=True,
                   cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return open(out).read()


def _kernels(text, fragment):
    """-> [(symbol, body: the instruction lines, meta: the metadata as a dict)] of the kernels whose mangled name contains `fragment`."""
    notes = text[text.index('amdhsa.kernels:'):]
    blocks = re.split(r'^  - (?=\.)', notes, flags=re.M)
    out = []
    for m in re.finditer(r'^(\w*%s\w*):' % fragment, text, re.M):
        sym = m.group(1)
        body = text[m.end():]
        body = body[:body.index('s_endpgm')]
        mine = [b for b in blocks if re.search(r'^\s*\.name:\s+%s\s*$' % re.escape(sym), b, re.M)]
        assert len(mine) == 1, sym
        out.append((sym, body, {k: int(v) for k, v in re.findall(r'^\s*\.(\w+):\s+(\d+)\s*$', mine[0], re.M)}))
    assert out, fragment
    return out


def _kernel(text, fragment):
    """-> (body, meta) of the one kernel whose mangled name contains `fragment`."""
    (_, body, meta), = _kernels(text, fragment)
    return body, meta


@pytest.fixture(scope='module')
def m16(tmp_path_factory):
    return _kernel(_compile('mlp16.hip', tmp_path_factory.mktemp('m16')), 'canonical_mlp_lds_kernel')


@pytest.fixture(scope='module')
def nr16(tmp_path_factory):
    return _kernel(_compile('nonrigid16.hip', tmp_path_factory.mktemp('nr16')), 'nonrigid_lds_kernel')


SELF_MAX = re.compile(r'\bv_max_f32(?:_e32|_e64)?\s+v\d+,\s*(v\d+),\s*\1\b')


def _footprint(meta, waves_per_simd, spills=0, scratch=0):
    assert meta['vgpr_spill_count'] <= spills
    assert meta['private_segment_fixed_size'] <= scratch
    assert meta['vgpr_count'] <= 512 // waves_per_simd           # 512 registers per SIMD lane
    assert meta['group_segment_fixed_size'] <= 163840 // waves_per_simd      # 4-wave workgroups: as many per CU (160 KiB of LDS)


def _check(body, meta):
    # a ReLU of an accumulator is ONE instruction: no self-max that quiets a signalling NaN in front of it
    assert SELF_MAX.search('\tv_max_f32_e32 v0, v54, v54\n') and not SELF_MAX.search('\tv_max_f32_e32 v162, 0, v0\n')
    assert SELF_MAX.findall(body) == []
    _footprint(meta, 2)          # no spill, no scratch, two waves per SIMD, two workgroups per CU


def _ring(body):
    """-> static (MFMAs, chunk barriers, LDS-DMA pieces) of a kernel"""
    return tuple(len(re.findall(r'^\s*%s\b' % op, body, re.M)) for op in ('v_mfma_\\w+', 's_barrier', 'global_load_lds_dwordx4'))


def test_m16_kernel(m16):
    body, meta = m16
    _check(body, meta)
    # 7 200 executed per 16-sample tile; the six hidden layers share one unrolled body: no work added or lost
    assert len(re.findall(r'\bv_mfma_f32_16x16x4_f32\b', body)) == 2080
    assert _ring(body) == (2080, 36, 152)
    assert meta['group_segment_fixed_size'] == 78112             # 4 slots x 16 KiB + 3 144 floats of side data


def test_nr16_kernel(nr16):
    body, meta = nr16
    _check(body, meta)
    assert len(re.findall(r'\bv_mfma_f32_16x16x4_f32\b', body)) == 1312
    assert _ring(body) == (1312, 23, 52)
    assert meta['group_segment_fixed_size'] == 37392             # 4 slots x 8 KiB + 1 156 floats of side data


def test_split_and_trunk_kernels(tmp_path_factory):
    """The other three kernels on the ring: footprints that fit their launch bounds."""
    out = tmp_path_factory.mktemp('split')
    split = _kernels(_compile('mlp.hip', out), 'canonical_mlp_split_lds_kernel')
    assert len(split) == 3
    for _, body, meta in split:                                  # __launch_bounds__(256, 1)
        _footprint(meta, 1)
        assert _ring(body)[1:] == (51, 212)
    nr = _kernels(_compile('nonrigid.hip', out), 'nonrigid_split_kernel')
    assert len(nr) == 4
    for sym, body, meta in nr:                                   # __launch_bounds__(256, 2)
        if 'F16x3ELb1E' in sym:      # the watched f16x3 instantiation is at the 256-register cap and spills (48 registers, 196 B)
            _footprint(meta, 2, spills=48, scratch=196)
        else:
            _footprint(meta, 2)
        assert _ring(body)[1:] == (24, 104)
    (_, body, meta), = _kernels(_compile('trunks.hip', out), 'trunks_forward_kernel')      # __launch_bounds__(256, 1)
    _footprint(meta, 1)
    assert _ring(body) == (416, 28, 120)


def test_one_lds_dma_statement():
    """The LDS-DMA instruction is written in ONE place (weight_ring.h: glds16); comments may speak of it."""
    holders = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith(('.hip', '.h')):
            continue
        code = re.sub(r'//[^\n]*|/\*.*?\*/', '', open(os.path.join(CSRC, name)).read(), flags=re.S)
        if 'global_load_lds_dwordx4' in code:
            holders.append(name)
    assert holders == ['weight_ring.h']
