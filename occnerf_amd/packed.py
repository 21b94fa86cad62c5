"""`PackedMLPs`: the MFMA-ordered weights of the two MLPs and the one place that picks the kernel they go to.

cfg.mlp_precision selects the arithmetic of the renderer's two MLPs: 'fp32' (exact), or a split-operand mode whose kernels take
the weights as a second, 2-byte stream beside the fp32 one -- bf16 pieces ('bf16x3') or fp16 pieces with a scaled low part
('f16x3', fp32-grade: csrc/split.h).  The split-operand ops dispatch on that stream's dtype.

Every ops function is looked up on the `ops` module when it is called: bench.py, tests and tools replace them there.
"""
import copy

import torch
import torch.nn as nn

from . import ops

PRECISIONS = ('fp32', 'bf16x3', 'f16x3')


def _sources(cnl_mlp, nr_mlp):
    """(canonical weights, canonical biases, non-rigid Linear layers) in module order."""
    cw, cb = cnl_mlp.linear_params()
    return cw, cb, [m for m in nr_mlp.block_mlps if isinstance(m, nn.Linear)]


class PackedMLPs:
    """cnl, nr: the fp32 packs; cnl_split, nr_split: the 2-byte streams (None for fp32); nr_w0, nr_b0: the non-rigid MLP's first
    layer; domain_flag: the word the f16x3 kernels set when a hidden activation reaches the mode's clamp (4 094; csrc/split.h),
    None where nothing is watched; key: what the object was packed from (Network._packed_weights)."""

    @staticmethod
    def cache_key(cnl_mlp, nr_mlp, precision, domain_check):
        """Moves whenever a packed parameter changed (optimizer steps update the tensors in place: their `_version` counters
        move, whatever mode the module is in), or the precision or the domain-check mode did."""
        if precision not in PRECISIONS:
            raise RuntimeError(f"cfg.mlp_precision must be 'fp32', 'f16x3' or 'bf16x3', got {precision!r}")
        cw, cb, nr_lin = _sources(cnl_mlp, nr_mlp)
        srcs = cw + cb + [m.weight for m in nr_lin] + [m.bias for m in nr_lin]
        return (precision, str(domain_check)) + tuple((t.data_ptr(), t._version) for t in srcs)

    def __init__(self, cnl_mlp, nr_mlp, precision, domain_check):
        self.key = self.cache_key(cnl_mlp, nr_mlp, precision, domain_check)
        self.precision = precision
        cw, cb, nr_lin = _sources(cnl_mlp, nr_mlp)
        self._nr_weights = [m.weight.detach() for m in nr_lin]
        pack_c = {'bf16x3': ops.canonical_mlp_pack_bf16, 'f16x3': ops.canonical_mlp_pack_f16}.get(precision)
        pack_n = {'bf16x3': ops.nonrigid_pack_bf16, 'f16x3': ops.nonrigid_pack_f16}.get(precision)
        self.cnl = ops.canonical_mlp_pack(cw, cb)
        self.cnl_split = pack_c(cw) if pack_c else None
        self.nr = ops.nonrigid_pack(self._nr_weights, [m.bias.detach() for m in nr_lin])
        self.nr_split = pack_n(self._nr_weights) if pack_n else None
        self.nr_w0, self.nr_b0 = self._nr_weights[0], nr_lin[0].bias.detach()
        self.domain_flag = torch.zeros(1, device=cw[0].device, dtype=torch.int32) \
            if (precision == 'f16x3' and domain_check) else None
        self._nr_f16 = self.nr_split if precision == 'f16x3' else None

    def _view(self, **fields):
        view = copy.copy(self)          # (shallow: the same tensors)
        view.__dict__.update(fields)
        return view

    def exact(self):
        """The fp32 view of the same packs: nothing is packed again (the f16x3 fallback frame)."""
        return self._view(cnl_split=None, nr_split=None, domain_flag=None)

    def train_f16x3(self, domain_flag):
        """The view the bf16 training step takes its offsets from: the split-fp16 stream of the non-rigid MLP beside the fp32
        pack, whatever cfg.mlp_precision is (packed on first use, kept as long as this object), reporting into `domain_flag`."""
        if self._nr_f16 is None:
            self._nr_f16 = ops.nonrigid_pack_f16(self._nr_weights)
        return self._view(nr_split=self._nr_f16, domain_flag=domain_flag)

    def offsets(self, xyz, cond, hann, rows=None, count=None, out=None):
        """xyz + the non-rigid offset.  rows / count (list and count on the device): in place, for the listed samples only;
        otherwise every row, into `out` (a fresh tensor when None)."""
        if rows is not None:
            if self.nr_split is not None:
                return ops.nonrigid_bf16x3_rows(xyz, rows, count, cond, hann, self.nr_w0, self.nr_b0, self.nr, self.nr_split,
                                                domain_flag=self.domain_flag)
            return ops.nonrigid_rows(xyz, rows, count, cond, hann, self.nr_w0, self.nr_b0, self.nr)
        if self.nr_split is not None:
            return ops.nonrigid_bf16x3(xyz, cond, hann, self.nr_w0, self.nr_b0, self.nr, self.nr_split, out=out,
                                       domain_flag=self.domain_flag)
        return ops.nonrigid(xyz, cond, hann, self.nr_w0, self.nr_b0, self.nr, out=out)

    def canonical(self, mlp_in, raw, count=None, in_rows=None):
        """The canonical MLP of the first `count` feature rows (all of them when None) into raw[:, :4]; in_rows: see
        ops.canonical_mlp."""
        if self.cnl_split is not None:
            return ops.canonical_mlp_bf16x3(mlp_in, self.cnl, self.cnl_split, raw, count=count, in_rows=in_rows,
                                            domain_flag=self.domain_flag)
        return ops.canonical_mlp(mlp_in, self.cnl, raw, count=count, in_rows=in_rows)
