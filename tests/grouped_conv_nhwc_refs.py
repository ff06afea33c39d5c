"""References and cases for csrc/grouped_conv_nhwc.hip (kgdet_gconv3x3_nhwc_bf16) in plain numpy, no GPU:

    S[b, ho, wo, c] = sum_{ky, kx, i} x[b, ho s - 1 + ky, wo s - 1 + kx, g cpg + i] w[c][ky][kx][i],   g = c // cpg,
    raw:      y = bf16(S)
    epilogue: y = bf16([relu](fp32(bf16(S)) + bias[c]))      (a missing bias reads as 0)

x [B, H, W, C] and y [B, Ho, Wo, C] bf16, w [C][3][3][cpg] bf16, bias fp32.  The sum is tests/grouped_conv_refs.forward in
float64 on the NCHW view of the operands; the roundings are dense_refs.bf16_round_bits (integer arithmetic on the bits).

Exact tier.  x holds integers of [-3, 3] x 2^-3, w x 2^-6, bias x 2^-9: every product is a multiple of q = 2^-9, a sum has at
most 9 * 32 terms of at most 9 q -- 2592 q, far below 2^24 q -- so every partial sum in every order and tiling is an exact
float32 and the roundings to bf16 are the only inexact steps: a correct kernel returns the reference's bits.  Sums beyond 2^8 q
need more than bf16's 8 bits, so both roundings work, ties included (test_grouped_conv_nhwc_refs.py holds that a tie occurs).

Mixed tier.  Normal operands; a correct kernel's fp32 accumulation lies within e = 9 cpg 2^-23 sum |x w| of the float64 sum
(any order, exact products, a unit roundoff that covers a truncating adder: the bound of tests/nhwc_refs.py) and the map from the
sum to the output is monotone, so every element must lie in [final(S - e), final(S + e)]; where both ends are one bf16 -- all
but the share pinned in MIXED_AMBIGUOUS -- that is bit equality.
"""
import collections
import functools
import zlib

import numpy as np

from tests import grouped_conv_refs as G
from tests.dense_refs import bf16_round_bits

f32 = np.float32
CPGS = G.CPGS
SMALL_MAPS = G.SMALL_MAPS                     # every border combination, odd sizes at stride 2
LARGE_MAPS = ((17, 33), (33, 65))             # one past a power-of-two tile: several 8 x 16 / 4 x 16 tiles, ragged both ways
GROUPS = {4: (2, 6, 32), 8: (1, 3), 16: (1, 3), 32: (1, 3)}       # C % 8 == 0; C % 16 == 8 at cpg 4 and 8; 128 and 96: two slabs
MODES = ('raw', 'bias', 'bias_relu', 'relu')

Case = collections.namedtuple('Case', 'name cpg stride groups B H W')


def _case(cpg, stride, groups, B, H, W, tag=''):
    return Case('%sc%d_s%d_g%d_b%d_%dx%d' % (tag, cpg, stride, groups, B, H, W), cpg, stride, groups, B, H, W)


def _cases():
    cases, i = [], 0
    for cpg in CPGS:
        for stride in (1, 2):
            for H, W in SMALL_MAPS + LARGE_MAPS:
                groups, B = GROUPS[cpg][i % len(GROUPS[cpg])], (1, 3)[(i // 2) % 2]
                i += 1
                cases.append(_case(cpg, stride, groups, B, H, W))
    # the kernel's own seams.  A workgroup owns a slab of 64 channels: a slab that ends inside a 16-channel block (72), inside a
    # wave's share (80), and a second slab of one group (cpg 32: 96 is in the table above)
    cases += [_case(8, 1, 9, 1, 5, 7, 'slab_'), _case(8, 2, 9, 1, 5, 7, 'slab_'), _case(16, 1, 5, 1, 5, 7, 'slab_'),
              _case(4, 2, 18, 1, 5, 7, 'slab_')]
    # a workgroup walks the tiles (batch x 8 x 16 outputs at stride 1, 4 x 16 at stride 2) in as many trips as keep a launch at
    # 4096 / slabs workgroups: 700 * 2 * 3 = 4200 and 1040 * 2 * 2 = 4160 tiles of one slab are two trips per workgroup
    cases += [_case(4, 1, 2, 700, 9, 33, 'trip_'), _case(4, 2, 2, 1040, 9, 33, 'trip_')]
    return cases


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
out_size = G.out_size


# ---------------------------------------------------------------------------------------------- layouts
def to_nhwc(a):
    """[B, C, H, W] -> [B, H, W, C], contiguous"""
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def to_nchw(a):
    """[B, H, W, C] -> [B, C, H, W], contiguous"""
    return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))


def pack_weight(w):
    """[C, cpg, 3, 3] -> [C][3][3][cpg]: the channels-last storage of the weight tensor"""
    return np.ascontiguousarray(np.transpose(w, (0, 2, 3, 1)))


def unpack_weight(wp):
    """[C][3][3][cpg] -> [C, cpg, 3, 3]"""
    return np.ascontiguousarray(np.transpose(wp, (0, 3, 1, 2)))


def bf16_bits(v):
    """the 16 bits of float32 values that ARE bf16 numbers"""
    u = np.ascontiguousarray(v, f32).view(np.uint32)
    assert not (u & 0xffff).any(), 'not a bf16 number'
    return (u >> 16).astype(np.uint16)


def from_bf16_bits(b):
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(f32)


# ---------------------------------------------------------------------------------------------- the operation
def sum64(x_nhwc, w_packed, stride):
    """S [B, Ho, Wo, C] in float64 of x [B, H, W, C] and w [C][3][3][cpg]"""
    return to_nhwc(G.forward(to_nchw(x_nhwc), unpack_weight(w_packed), stride))


def final_raw(s):
    """the raw store: bf16 of the fp32 sum; monotone in s"""
    return bf16_round_bits(np.asarray(s).astype(f32))


def final_epilogue(s, bias=None, relu=False):
    """the epilogue store: bf16([relu](fp32(bf16(s)) + bias[c])), channels last, the addition in float32; monotone in s"""
    f = bf16_round_bits(np.asarray(s).astype(f32))
    if bias is not None:
        f = f + np.asarray(bias, f32)
    if relu:
        f = np.maximum(f, f32(0))
    return bf16_round_bits(f)


def final(s, mode, bias):
    if mode == 'raw':
        return final_raw(s)
    return final_epilogue(s, bias if mode in ('bias', 'bias_relu') else None, mode in ('bias_relu', 'relu'))


# ---------------------------------------------------------------------------------------------- exact tier
XE, WE, BE = -3, -6, -9
Operands = collections.namedtuple('Operands', 'x w bias')       # x [B, H, W, C], w [C][3][3][cpg], bias [C], float32


@functools.lru_cache(maxsize=None)
def lattice(name):
    c = BY_NAME[name]
    rng = np.random.default_rng(zlib.crc32(repr(('nhwc lattice', name)).encode()))
    C = c.groups * c.cpg

    def ints(shape, e):
        return (rng.integers(-3, 4, shape).astype(np.float64) * 2.0 ** e).astype(f32)
    op = Operands(ints((c.B, c.H, c.W, C), XE), ints((C, 3, 3, c.cpg), WE), ints((C,), BE))
    for v in op:
        v.setflags(write=False)
    return op


@functools.lru_cache(maxsize=None)
def lattice_sum(name):
    """(S in float64, the largest sum of |terms| in quanta of 2^-9)"""
    c, op = BY_NAME[name], lattice(name)
    S = sum64(op.x, op.w, c.stride)
    mag = sum64(np.abs(op.x), np.abs(op.w), c.stride)
    S.setflags(write=False)
    return S, float(mag.max() / 2.0 ** (XE + WE))


def lattice_reference(name, mode):
    """the bits a correct kernel returns: float32 array of bf16 values [B, Ho, Wo, C]"""
    S, _ = lattice_sum(name)
    return final(S, mode, lattice(name).bias)


def ties(name):
    """how many sums of the case sit exactly between two bf16 numbers"""
    S, _ = lattice_sum(name)
    u = S.astype(f32).view(np.uint32)
    return int(((u & 0xffff) == 0x8000).sum())


# ---------------------------------------------------------------------------------------------- mixed tier
MIXED_G, MIXED_B, MIXED_H, MIXED_W = 4, 2, 17, 33
MIXED_MODES = ('raw', 'bias', 'bias_relu')
MIXED_CAP = 0.35
# the share of elements whose interval ends differ, (cpg, stride) -> (raw, bias, bias + ReLU), as computed on the CPU with the
# recipe of mixed_inputs; every element outside it is held bit-exact.  It grows with the length of the sum (e grows as
# cpg^1.5 against the output's spacing), shrinks with the bias (a wider output) and halves with the ReLU.
MIXED_AMBIGUOUS = {
    (4, 1): (0.027, 0.005, 0.003), (4, 2): (0.029, 0.007, 0.004),
    (8, 1): (0.066, 0.022, 0.011), (8, 2): (0.066, 0.020, 0.011),
    (16, 1): (0.152, 0.068, 0.036), (16, 2): (0.145, 0.064, 0.031),
    (32, 1): (0.321, 0.199, 0.097), (32, 2): (0.318, 0.200, 0.097),
}
MIXED_CASES = [(cpg, s) for cpg in CPGS for s in (1, 2)]


@functools.lru_cache(maxsize=None)
def mixed_inputs(cpg, stride):
    rng = np.random.default_rng([cpg, stride, 33])
    C = MIXED_G * cpg
    x = bf16_round_bits(rng.standard_normal((MIXED_B, C, MIXED_H, MIXED_W)).astype(f32))
    w = bf16_round_bits((0.1 * rng.standard_normal((C, cpg, 3, 3))).astype(f32))
    bias = rng.standard_normal(C).astype(f32)
    op = Operands(to_nhwc(x), pack_weight(w), bias)
    for v in op:
        v.setflags(write=False)
    return op


@functools.lru_cache(maxsize=None)
def mixed_interval(cpg, stride):
    """{mode: dict(lo, hi: float32 arrays of bf16 values [B, Ho, Wo, C]; ambiguous: the share of elements with lo != hi)}"""
    op = mixed_inputs(cpg, stride)
    S = sum64(op.x, op.w, stride)
    e = 9 * cpg * 2.0 ** -23 * sum64(np.abs(op.x), np.abs(op.w), stride)
    out = {}
    for mode in MIXED_MODES:
        lo, hi = final(S - e, mode, op.bias), final(S + e, mode, op.bias)
        assert (lo <= hi).all()
        out[mode] = dict(lo=lo, hi=hi, ambiguous=float((bf16_bits(lo) != bf16_bits(hi)).mean()))
    return out
