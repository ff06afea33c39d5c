"""The bf16 channels-last grouped 3x3 convolution -- csrc/grouped_conv_nhwc.hip, kgdet_gconv3x3_nhwc_bf16 -- through the C ABI
against tests/grouped_conv_nhwc_refs.py.

The output is prefilled with bf16 NaN (0x7FC0) and sits between canaries; the activation, the weight and the bias sit between
NaN-filled guard regions of a larger buffer, so a read outside them that reaches a sum shows up as NaN.

  exact   lattice operands: the reference's bits for raw, bias, bias + ReLU and ReLU alone;
  mixed   normal operands: every element inside [final(S - e), final(S + e)], e = 9 cpg 2^-23 sum |x w| -- bit equality wherever
          the two ends are one bf16; where the ambiguous elements landed is printed per case.
"""
import numpy as np
import pytest
import torch

from tests import grouped_conv_nhwc_refs as R
from tests.test_gpu_step_kernels import Guarded

pytestmark = pytest.mark.gpu

OK, E_SHAPE = 0, 1
GUARD = 64                  # elements: 128 bytes of bf16, 256 of fp32 -- the payload keeps its 16-byte alignment
NAN16 = 0x7FC0


def _L():
    from kgdet_amd import grouped_conv
    return grouped_conv.library()


def _st():
    from kgdet_amd import _lib
    return _lib.raw_stream()


class _In16(object):
    """bf16 numbers (given as float32) between two guard regions of bf16 NaN"""

    def __init__(self, a):
        bits = R.bf16_bits(a).reshape(-1).astype(np.int16)
        self.n = bits.size
        self.buf = torch.full((2 * GUARD + bits.size,), NAN16, dtype=torch.int16, device='cuda')
        self.buf[GUARD:GUARD + bits.size] = torch.from_numpy(bits).cuda()
        self.ptr = self.buf.data_ptr() + 2 * GUARD
        assert self.ptr % 16 == 0

    def payload(self):
        return self.buf[GUARD:GUARD + self.n].clone()


class _In32(object):
    """float32 numbers between two guard regions of NaN"""

    def __init__(self, a):
        a = np.array(a, np.float32).reshape(-1)
        self.buf = torch.full((2 * GUARD + a.size,), float('nan'), dtype=torch.float32, device='cuda')
        self.buf[GUARD:GUARD + a.size] = torch.from_numpy(a).cuda()
        self.ptr = self.buf.data_ptr() + 4 * GUARD
        assert self.ptr % 16 == 0


class _Out16(object):
    """n bf16 elements (n even) of NaN between the canaries of a Guarded float buffer"""

    def __init__(self, n):
        assert n % 2 == 0
        self.n, self.g = n, Guarded(n // 2)
        self.g.view().view(torch.int16).fill_(NAN16)
        self.ptr = self.g.buf.data_ptr() + 4 * self.g.lead
        assert self.ptr % 16 == 0

    def bits(self, shape):
        return self.g.view().view(torch.int16).cpu().numpy().view(np.uint16).reshape(shape)

    def untouched(self):
        return self.g.intact() and bool((self.g.view().view(torch.int16) == NAN16).all())


class _Run(object):
    def __init__(self, cpg, stride, B, H, W, op):
        self.cpg, self.stride, self.B, self.H, self.W = cpg, stride, B, H, W
        self.C = op.x.shape[3]
        assert op.x.shape == (B, H, W, self.C) and op.w.shape == (self.C, 3, 3, cpg)
        self.y_shape = (B, R.out_size(H, stride), R.out_size(W, stride), self.C)
        self.x, self.w, self.bias = _In16(op.x), _In16(op.w), _In32(op.bias)

    def call(self, mode, out=None, **change):
        y = out or _Out16(int(np.prod(self.y_shape)))
        a = dict(x=self.x.ptr, w=self.w.ptr, bias=self.bias.ptr if mode in ('bias', 'bias_relu') else None, y=y.ptr, B=self.B,
                 C=self.C, cpg=self.cpg, H=self.H, W=self.W, stride=self.stride, relu=1 if mode in ('bias_relu', 'relu') else 0)
        a.update(change)
        rc = _L().kgdet_gconv3x3_nhwc_bf16(a['x'], a['w'], a['bias'], a['y'], a['B'], a['C'], a['cpg'], a['H'], a['W'],
                                           a['stride'], a['relu'], _st())
        return rc, y

    def bits(self, mode):
        rc, y = self.call(mode)
        assert rc == OK and y.g.intact()
        return y.bits(self.y_shape)


def _of_case(name):
    c = R.BY_NAME[name]
    return _Run(c.cpg, c.stride, c.B, c.H, c.W, R.lattice(name))


def _same_bits(got, ref, tag):
    want = R.bf16_bits(ref)
    bad = (got != want) & ~(((got & 0x7fff) == 0) & ((want & 0x7fff) == 0))       # (a zero of either sign is a zero)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError('%s: %d of %d elements differ, first at [b, ho, wo, c] = %s: got %r, want %r' % (
            tag, int(bad.sum()), bad.size, at, float(R.from_bf16_bits(got[at])), float(ref[at])))


@pytest.mark.parametrize('name', R.NAMES)
def test_exact_tier_returns_the_references_bits(name):
    run = _of_case(name)
    for mode in R.MODES:
        _same_bits(run.bits(mode), R.lattice_reference(name, mode), '%s %s' % (name, mode))


@pytest.mark.parametrize('cpg,stride', R.MIXED_CASES)
def test_mixed_tier_stays_inside_the_interval_of_its_float64_sum(cpg, stride):
    op, iv = R.mixed_inputs(cpg, stride), R.mixed_interval(cpg, stride)
    run = _Run(cpg, stride, R.MIXED_B, R.MIXED_H, R.MIXED_W, op)
    for mode in R.MIXED_MODES:
        lo, hi = iv[mode]['lo'], iv[mode]['hi']
        bits = run.bits(mode)
        got = R.from_bf16_bits(bits)
        assert np.isfinite(got).all(), 'non-finite results (a read outside an operand?)'
        open_ = R.bf16_bits(lo) != R.bf16_bits(hi)
        at_lo, at_hi = int((open_ & (got == lo)).sum()), int((open_ & (got == hi)).sum())
        print('cpg %d stride %d %-9s: %d of %d elements ambiguous (%.4f): %d at the lower end, %d at the upper, %d between'
              % (cpg, stride, mode, int(open_.sum()), open_.size, open_.mean(), at_lo, at_hi, int(open_.sum()) - at_lo - at_hi))
        outside = (got < lo) | (got > hi)
        assert not outside.any(), '%d of %d elements outside their interval, first at %s' % (
            int(outside.sum()), outside.size, np.argwhere(outside)[0])
        _same_bits(np.where(open_, 0, bits).astype(np.uint16), np.where(open_, np.float32(0), lo), 'cpg %d stride %d %s' % (cpg, stride, mode))


@pytest.mark.parametrize('name', ['c4_s1_g6_b3_33x65', 'c32_s2_g3_b3_33x65', 'trip_c4_s1_g2_b700_9x33'])
def test_two_calls_give_equal_bits(name):
    assert name in R.BY_NAME
    run = _of_case(name)
    for mode in ('raw', 'bias_relu'):
        assert np.array_equal(run.bits(mode), run.bits(mode))


def test_every_refusal_leaves_the_output_untouched():
    name = 'c8_s1_g3_b3_33x65'
    run = _of_case(name)
    x_before, w_before = run.x.payload(), run.w.payload()
    y = _Out16(int(np.prod(run.y_shape)))
    changes = [dict(cpg=2), dict(cpg=64), dict(stride=3), dict(stride=0), dict(C=run.C + 4), dict(C=12, cpg=4), dict(x=None),
               dict(w=None), dict(x=run.x.ptr + 2), dict(x=run.x.ptr + 8), dict(w=run.w.ptr + 8), dict(bias=run.bias.ptr + 4),
               dict(y=y.ptr + 8), dict(B=0), dict(W=0)]
    for change in changes:
        rc, _ = run.call('bias_relu', out=y, **change)
        assert rc == E_SHAPE, change
        assert b'gconv3x3_nhwc_bf16' in _L().kgdet_last_error(), change
        assert y.untouched(), change
    # a null y, and a y that overlaps an operand: nothing is written anywhere
    for change in (dict(y=None), dict(y=run.x.ptr), dict(y=run.x.ptr + 16), dict(y=run.w.ptr), dict(y=run.bias.ptr)):
        rc, _ = run.call('bias_relu', out=y, **change)
        assert rc == E_SHAPE, change
    torch.cuda.synchronize()
    assert torch.equal(run.x.payload(), x_before) and torch.equal(run.w.payload(), w_before) and y.untouched()
    # and the same arguments unchanged are taken
    rc, y2 = run.call('bias_relu')
    assert rc == OK
    _same_bits(y2.bits(run.y_shape), R.lattice_reference(name, 'bias_relu'), name)
