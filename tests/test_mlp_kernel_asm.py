"""CPU: what the compiler makes of the two fp32 LDS-staged MLP kernels (mlp16.hip, nonrigid16.hip).

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


def _kernel(text, fragment):
    """-> (body: the instruction lines of the kernel whose mangled name contains `fragment`, meta: its metadata as a dict)."""
    m = re.search(r'^(\w*%s\w*):' % fragment, text, re.M)
    assert m, fragment
    sym = m.group(1)
    body = text[m.end():]
    body = body[:body.index('s_endpgm')]
    notes = text[text.index('amdhsa.kernels:'):]
    blocks = re.split(r'^  - (?=\.)', notes, flags=re.M)
    mine = [b for b in blocks if re.search(r'^\s*\.name:\s+%s\s*$' % re.escape(sym), b, re.M)]
    assert len(mine) == 1, sym
    meta = {k: int(v) for k, v in re.findall(r'^\s*\.(\w+):\s+(\d+)\s*$', mine[0], re.M)}
    return body, meta


@pytest.fixture(scope='module')
def m16(tmp_path_factory):
    return _kernel(_compile('mlp16.hip', tmp_path_factory.mktemp('m16')), 'canonical_mlp_lds_kernel')


@pytest.fixture(scope='module')
def nr16(tmp_path_factory):
    return _kernel(_compile('nonrigid16.hip', tmp_path_factory.mktemp('nr16')), 'nonrigid_lds_kernel')


SELF_MAX = re.compile(r'\bv_max_f32(?:_e32|_e64)?\s+v\d+,\s*(v\d+),\s*\1\b')


def _check(body, meta):
    # a ReLU of an accumulator is ONE instruction: no self-max that quiets a signalling NaN in front of it
    assert SELF_MAX.search('\tv_max_f32_e32 v0, v54, v54\n') and not SELF_MAX.search('\tv_max_f32_e32 v162, 0, v0\n')
    assert SELF_MAX.findall(body) == []
    assert meta['vgpr_spill_count'] == 0
    assert meta['private_segment_fixed_size'] == 0              # no scratch
    assert meta['vgpr_count'] <= 256                            # two waves per SIMD
    assert meta['group_segment_fixed_size'] <= 81920            # two workgroups per CU (160 KiB of LDS)


def test_m16_kernel(m16):
    body, meta = m16
    _check(body, meta)
    # 7 200 executed per 16-sample tile; the six hidden layers share one unrolled body: no work added or lost
    assert len(re.findall(r'\bv_mfma_f32_16x16x4_f32\b', body)) == 2080


def test_nr16_kernel(nr16):
    _check(*nr16)
