"""References of the dense convolutions (csrc/dense_forward.hip, dense_grad_weight.hip): the operand split restated with torch's
casts, the float64 sum S3 of exactly the three products the kernels form, operand generators, and the table of shapes -- one row
per branch of plan_nn / plan_gw with the plan it must take.

Plain numpy / CPU torch, no GPU.  tests/test_dense_refs.py pins all of it; tests/test_gpu_dense_kernels.py holds the kernels to it
through the C ABI, in three tiers:

  exact         operands on an integer lattice (small integers times a power of two, a sprinkling of "wide" values whose split is
                exact with a non-zero lo part): every term of every output is a multiple of one quantum q and sum |terms| <
                2^24 q, so every partial sum in every order is an exact float and every correct kernel -- whatever its tile shape,
                K split or summation order -- returns the bits of S3;
  accumulation  mixed-scale operands: a kernel differs from S3 by its fp32 accumulation only, measured per normalisation group
                (output channel, weight-gradient row, image) against ACC_BAR;
  envelope      S3 differs from the exact float64 convolution by the split only, deterministically: what the number formats give,
                per group, computed here on the CPU.
"""
import collections
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

BF16, FP16 = 0, 1                      # operand_format of the *_fmt entry points
F16_MAX = 65504.0
F16_WEIGHT_SCALE = 256.0               # csrc/dense_common.h kF16WeightScale
WIDE = {BF16: 257.0, FP16: 2049.0}     # hi = 256 / 2048 (round to nearest even), lo = 1
ACC_BAR = 1e-6                         # the suite's fp32-class figure (test_fp16_forward_parts_envelope)
SPLIT_BAR = {BF16: 1e-5, FP16: 1e-6}   # the suite's bars on S3 - exact: bf16 parts leave ~5e-6 of the output scale, fp16 parts 1e-6
# The envelope tier holds bf16 backward results to SPLIT_BAR per group against the exact float64 result.  The bar is the suite's
# figure for whole tensors; what the split itself leaves per term is bounded by 3 x 2^-18 = 1.14e-5 of |a b| (hi and lo each round
# to 8 bits: |v - hi - lo| <= 2^-18 |v|, and the dropped a_lo b_lo <= 2^-18 |a b|), so a group made of a few short sums can exceed
# the bar by the format alone.  The assertion is made where S3 - exact (computed on the CPU) leaves the accumulation bar of room;
# the cases where it does not are named here with that figure pinned by tests/test_dense_refs.py, and stay held to S3.
ENVELOPE_ROOM = SPLIT_BAR[BF16] - ACC_BAR
BF16_SPLIT_OVER = {          # weight-gradient case: S3 - exact per row, of the row's max (mixed-scale operands)
    'nt8_1': 9.4e-6,         # 512 pixels, half of them masked, 128 columns per row: no room left
    'nt8_1_padded': 1.7e-5,  # 3 pixels per image: a row's elements are sums of <= 6 products
    'nt8_9_padded': 1.1e-5,  # 15 pixels per image
}
# fp16 parts, weights: the image holds w * 2^8; the lo part is a normal fp16 number (>= 2^-14) while |w| * 2^8 * 2^-11 >= 2^-14
F16_WEIGHT_NORMAL_LO = 2.0 ** -11


# ---------------------------------------------------------------------------------------------- the operand split
def split(v, fmt):
    """(hi, lo) of float32 ``v`` as the kernels form them (dense_common.h split_pair / split_pair_t): hi = fmt(v),
    lo = fmt(v - hi), round to nearest even; fp16 parts clamped to +-65504 (f16_saturate_on)"""
    v = torch.as_tensor(v, dtype=torch.float32)
    if fmt == BF16:
        hi = v.to(torch.bfloat16).float()
        lo = (v - hi).to(torch.bfloat16).float()
    else:
        hi = v.to(torch.float16).float().clamp(-F16_MAX, F16_MAX)
        lo = (v - hi).to(torch.float16).float().clamp(-F16_MAX, F16_MAX)
    return hi, lo


def split_weight(w, fmt):
    """parts of a packed weight and the factor the kernel takes out of its accumulators again"""
    w = torch.as_tensor(w, dtype=torch.float32)
    if fmt == FP16:
        return split(w * np.float32(F16_WEIGHT_SCALE), FP16) + (1.0 / F16_WEIGHT_SCALE,)
    return split(w, BF16) + (1.0,)


def bf16_round_bits(v):
    """bf16(v) as float32 by integer arithmetic on the bits (finite v): independent of torch's cast"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


# ---------------------------------------------------------------------------------------------- the bilinear operations, float64
Op = collections.namedtuple('Op', 'fn b_is_weight')     # fn(a, b) in float64, bilinear; b_is_weight: b goes through split_weight


def op_forward(k, stride):
    """y = conv(x, w): x [B, K, H, W], w [M, K, k, k], padding k // 2 (1x1, 3x3, the 7x7 stem)"""
    return Op(lambda x, w: F.conv2d(x, w, stride=stride, padding=k // 2), True)


def op_grad_input(k, stride, Hin, Win):
    """gx [B, C, Hin, Win] = conv_transpose(gy, w), w [O, C, k, k]: the transposed operand with mirrored taps; stride 2 scatters into
    the four parity classes of the input pixels"""
    def fn(gy, w):
        H, W = gy.shape[2], gy.shape[3]
        opad = (Hin - ((H - 1) * stride + 1), Win - ((W - 1) * stride + 1)) if stride == 2 else 0
        return F.conv_transpose2d(gy, w, stride=stride, padding=k // 2, output_padding=opad)
    return Op(fn, True)


def op_grad_weight(k, stride, C):
    """gw [O, C, k, k] = sum over images and pixels of gy [B, O, Ho, Wo] x patches(x [B, C, H, W])"""
    def fn(gy, x):
        O = gy.shape[1]
        return torch.nn.grad.conv2d_weight(x, (O, C, k, k), gy, stride=stride, padding=k // 2)
    return Op(fn, False)


def _parts(op, a, b, fmt):
    ah, al = split(a, fmt)
    if op.b_is_weight:
        bh, bl, scale = split_weight(b, fmt)
    else:
        (bh, bl), scale = split(b, fmt), 1.0
    return [t.double() for t in (ah, al, bh, bl)], scale


def s3(op, a, b, fmt):
    """float64 sum of exactly the three products the kernels form: a_hi b_hi + a_hi b_lo + a_lo b_hi"""
    (ah, al, bh, bl), scale = _parts(op, a, b, fmt)
    return (op.fn(ah, bh) + op.fn(ah, bl) + op.fn(al, bh)) * scale


def lolo(op, a, b, fmt):
    """the product the kernels drop: a_lo b_lo"""
    (ah, al, bh, bl), scale = _parts(op, a, b, fmt)
    return op.fn(al, bl) * scale


def exact(op, a, b):
    """the float64 operation on the float32 operands"""
    return op.fn(torch.as_tensor(a, dtype=torch.float32).double(), torch.as_tensor(b, dtype=torch.float32).double())


def abs_terms(op, a, b, fmt):
    """sum of |terms| of every output element over the three products (an upper bound of it: all four)"""
    (ah, al, bh, bl), scale = _parts(op, a, b, fmt)
    return op.fn(ah.abs() + al.abs(), bh.abs() + bl.abs()) * scale


def group_max(ref, axis):
    """max |ref| per normalisation group, broadcastable against ref: ``axis`` is the group's axis"""
    r = np.abs(np.asarray(ref, np.float64))
    other = tuple(i for i in range(r.ndim) if i != axis)
    return r.max(axis=other, keepdims=True)


def group_ratio(got, ref, axis):
    """max over the groups of max |got - ref| / max |ref| (a group whose reference is all zero must be all zero: inf otherwise)"""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    other = tuple(i for i in range(err.ndim) if i != axis)
    e, m = err.max(axis=other), group_max(ref, axis).reshape(-1)
    with np.errstate(all='ignore'):
        r = np.where(e == 0, 0.0, e / m)
    return float(r.max())


# ---------------------------------------------------------------------------------------------- the case table
# kernel: nn<taps>w<waves> = conv_nn<taps, waves>, p<waves><blocks> = conv3x3_patch4<waves, blocks> (p24: the 64-row halves)
# closer (plan word 9, epilogue flags given): 0 the kernel's store, 1 conv1x1_sum_epilogue, 2 conv1x1_sum + kgdet_bias_act
# transpose: the weight is [K, M, k, k] and packed as the grad_input image (stride 1 grad_input runs the forward kernels, bf16 parts)
FwdCase = collections.namedtuple('FwdCase', 'name B M K H W taps stride kernel ks closer transpose')


def _f(name, B, M, K, H, W, taps, stride, kernel, ks, closer, transpose=False):
    return FwdCase(name, B, M, K, H, W, taps, stride, kernel, ks, closer, transpose)


# one row per branch of plan_nn (the plan columns are unique)
FWD_BRANCHES = [
    _f('nn1_store', 1, 128, 112, 12, 11, 1, 1, 'nn1w4', 1, 0),             # 7 stages: ks == 1 without trying
    _f('nn1_ks2_uneven', 1, 128, 272, 12, 11, 1, 1, 'nn1w4', 2, 1),        # 17 stages: parts of 9 + 8
    _f('nn1_ks8', 1, 128, 1040, 12, 11, 1, 1, 'nn1w4', 8, 1),              # 65 stages: parts of 9 x 7 + 2
    _f('nn1_ks2_odd', 1, 128, 272, 11, 13, 1, 1, 'nn1w4', 2, 2),           # 143 pixels: conv1x1_sum, then kgdet_bias_act
    _f('nn1_w5', 2, 136, 16, 84, 100, 1, 1, 'nn1w5', 1, 0),                # 264 tiles of 128 pixels, 212 of 160
    _f('nn1_s2_ks2', 1, 128, 272, 24, 22, 1, 2, 'nn1w4', 2, 1),
    _f('nn9_s2_store', 2, 40, 16, 14, 9, 9, 2, 'nn9w4', 1, 0),
    _f('nn9_s2_ks2', 1, 128, 32, 13, 11, 9, 2, 'nn9w4', 2, 1),
    _f('nn9_w5', 2, 136, 16, 168, 200, 9, 2, 'nn9w5', 1, 0),               # the same output pixels as nn1_w5, at stride 2
    _f('p44_store', 1, 128, 32, 21, 19, 9, 1, 'p44', 1, 0),                # 10 x 12 tiles: ragged right and bottom
    _f('p44_ks2', 1, 128, 64, 12, 12, 9, 1, 'p44', 2, 1),
    _f('p44_ks8_odd', 1, 96, 512, 11, 13, 9, 1, 'p44', 8, 2),              # the longest reduction: 3x3, K = 512
    _f('p24_m64', 2, 64, 32, 37, 5, 9, 1, 'p24', 1, 0),                    # M <= 64; a map narrower than 8 columns
    _f('p24_tiles', 1, 80, 16, 163, 245, 9, 1, 'p24', 1, 0),               # 256 < 328 tiles < 400 with ks == 1
    _f('p45', 1, 136, 16, 83, 194, 9, 1, 'p45', 1, 0),                     # 210 tiles of 160 pixels against 264 of 128
    _f('gi1', 2, 130, 112, 12, 11, 1, 1, 'nn1w4', 1, 0, True),             # grad_input of a 1x1 [112 -> 130]
    _f('gi9', 1, 72, 32, 21, 19, 9, 1, 'p44', 1, 0, True),                 # grad_input of a 3x3 [32 -> 72]: mirrored taps
]
# further shapes on branches already listed: channel counts either side of 32 / 64 / 128, ragged K, odd M with an even product
FWD_EDGES = [
    _f('nn1_m33_k13', 1, 33, 13, 12, 11, 1, 1, 'nn1w4', 1, 0),
    _f('nn1_m65_k166', 1, 65, 166, 12, 12, 1, 1, 'nn1w4', 1, 0),
    _f('nn1_m129_k588', 2, 129, 588, 10, 10, 1, 1, 'nn1w4', 4, 1),
    _f('nn1_m31_k31', 2, 31, 31, 8, 8, 1, 1, 'nn1w4', 1, 0),
    _f('nn1_s2_m33_k13', 1, 33, 13, 23, 21, 1, 2, 'nn1w4', 1, 0),
    _f('p24_m31_k48', 1, 31, 48, 9, 10, 9, 1, 'p24', 1, 0),
    _f('p44_m127_k16', 1, 127, 16, 7, 30, 9, 1, 'p44', 1, 0),              # a map of 7 rows
    _f('p44_m200_k64', 1, 200, 64, 12, 12, 9, 1, 'p44', 2, 1),             # two row tiles, the second ragged
]
FWD_CASES = FWD_BRANCHES + FWD_EDGES
FWD_BY_NAME = {c.name: c for c in FWD_CASES}
CLOSER_CASES = ['nn1_store', 'nn1_ks2_uneven', 'nn1_ks2_odd', 'p44_ks2']    # the three closing passes (and the patch kernel's)

# grad_input of the 3x3 stride-2 convolution: (B, C, O, Hin, Win), C no multiple of 128, every parity of the input map
S2GI_CASES = [(1, 72, 32, 13, 11), (2, 72, 16, 12, 10), (1, 40, 32, 13, 10), (1, 200, 16, 12, 11), (1, 72, 32, 37, 41), (1, 130, 16, 3, 2)]
STEM_CASES = [(2, 37, 45), (1, 64, 96), (1, 7, 5)]                       # (B, H, W): ragged, whole and smaller-than-one 8 x 16 tiles

# route: '1x1' | '3x3' | 's2' (kgdet_conv3x3_s2_grad_weight: C, H, W of its x; the plan is that of the 1x1 problem [O, 9 C, Ho Wo]);
# product: nt8 | ntp_aligned | ntp_ragged | nt8_padded; closers: the closing passes run on this shape, of
#   sum (conv1x1_sum) | wsum (conv3x3_wsum) | fold (conv_wsum_fold, bn_partial given) | fold_rows (... NULL: per-row sums of grad_y)
GwCase = collections.namedtuple('GwCase', 'name route B O C H W product splits closers')
GW_CASES = [
    GwCase('nt8_1', '1x1', 2, 128, 128, 1, 256, 'nt8', 1, ('sum', 'fold', 'fold_rows')),
    GwCase('nt8_1_splits', '1x1', 2, 130, 66, 1, 1000, 'nt8', 4, ('sum', 'fold_rows')),
    GwCase('ntp1_ragged', '1x1', 2, 128, 128, 1, 255, 'ntp_ragged', 1, ('sum', 'fold_rows')),
    GwCase('ntp1_ragged_splits', '1x1', 2, 70, 130, 1, 1051, 'ntp_ragged', 5, ('sum', 'fold', 'fold_rows')),
    GwCase('nt8_1_padded', '1x1', 2, 128, 128, 1, 3, 'nt8_padded', 1, ('sum', 'fold_rows')),
    GwCase('ntp9_aligned', '3x3', 2, 128, 128, 8, 12, 'ntp_aligned', 1, ('wsum', 'fold', 'fold_rows')),
    GwCase('ntp9_aligned_splits', '3x3', 2, 64, 128, 24, 28, 'ntp_aligned', 3, ('wsum', 'fold_rows')),
    GwCase('ntp9_ragged', '3x3', 2, 128, 128, 7, 9, 'ntp_ragged', 1, ('wsum', 'fold_rows')),
    GwCase('ntp9_ragged_splits', '3x3', 1, 130, 256, 25, 21, 'ntp_ragged', 2, ('wsum', 'fold', 'fold_rows')),
    GwCase('nt8_9_padded', '3x3', 2, 128, 128, 5, 3, 'nt8_padded', 1, ('wsum', 'fold_rows')),
    GwCase('s2_ragged', 's2', 2, 64, 40, 13, 11, 'ntp_ragged', 1, ('wsum',)),
    GwCase('s2_aligned', 's2', 2, 64, 40, 16, 12, 'nt8', 1, ('wsum',)),
]
GW_BY_NAME = {c.name: c for c in GW_CASES}
# Not in the table: conv_nt8<9> on maps beyond 2^21 pixels (plan_gw's route for what conv_ntp's float row index does not cover) --
# gigabyte operands.


def fwd_kernel_of(plan, taps):
    """the kernel name of a kgdet_conv_apply_plan answer (words: patch TX TY NB NW ks halves tiles n_nt closer closer_plain)"""
    if plan[0]:
        return 'p%d%d' % (2 if plan[6] else 4, plan[3])
    return 'nn%dw%d' % (taps, plan[4])


def gw_product_of(plan):
    """the product kernel of a kgdet_conv_grad_weight_plan answer (words: use_ntp padded aligned splits spi per ...)"""
    if plan[0]:
        return 'ntp_aligned' if plan[2] else 'ntp_ragged'
    return 'nt8_padded' if plan[1] else 'nt8'


def gw_plan_args(c):
    """(B, O, C, H, W, taps) of the plan query of a weight-gradient case"""
    if c.route == 's2':
        return c.B, c.O, 9 * c.C, 1, ((c.H + 1) // 2) * ((c.W + 1) // 2), 1
    return c.B, c.O, c.C, c.H, c.W, 9 if c.route == '3x3' else 1


# ---------------------------------------------------------------------------------------------- generators
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _small(rng, shape, e):
    """integers of [-3, 3] times 2^e"""
    return rng.integers(-3, 4, shape).astype(np.float64) * 2.0 ** e


def _sprinkle(rng, a, fmt, e, density):
    """wide values at a fraction ``density`` of the elements"""
    m = rng.random(a.shape) < density
    a[m] = rng.choice([-1.0, 1.0], int(m.sum())) * WIDE[fmt] * 2.0 ** e
    return a


def _rows_wide(rng, a, fmt, e, per_row):
    """``per_row`` wide values in every row a[i, ...] (the operand whose rows meet every element of the other)"""
    flat = a.reshape(a.shape[0], -1)
    for i in range(flat.shape[0]):
        j = rng.choice(flat.shape[1], min(per_row, flat.shape[1]), replace=False)
        flat[i, j] = rng.choice([-1.0, 1.0], len(j)) * WIDE[fmt] * 2.0 ** e
    return a


# exponents of the lattice: activations are integers x 2^EA, weights x 2^EW (fp16: 2049 x 2^-6 x 2^8 = 8196 stays inside the
# image's range and its lo part, 4, is normal), gradients x 2^EG (1e-9: where gradients live, far below fp16's range)
EA, EW, EG = -3, -6, -30
WIDE_DENSITY = 1.0 / 16      # of the activation-like operand
WIDE_PER_ROW = {BF16: 6, FP16: 2}    # of the row operand: at most this many wide x wide products per output (fp16: 2^22 q each)

Lattice = collections.namedtuple('Lattice', 'a b q bias residual gate')


def _f32(a):
    a32 = np.ascontiguousarray(a, np.float32)
    assert (a32.astype(np.float64) == a).all()
    return a32


@functools.lru_cache(maxsize=4)
def fwd_lattice(name, fmt):
    """x [B, K, H, W], w ([M, K, k, k], transpose: [K, M, k, k]), bias [M], residual and gate [B, M, Ho, Wo]; q the quantum of the
    products.  A transposed case carries gradient-sized activations."""
    c = FWD_BY_NAME[name]
    rng = _rng('fwd', name, fmt)
    k = 3 if c.taps == 9 else 1
    ea = EG if c.transpose else EA
    x = _sprinkle(rng, _small(rng, (c.B, c.K, c.H, c.W), ea), fmt, ea, WIDE_DENSITY)
    w = _small(rng, (c.M, c.K, k, k), EW)
    w = _rows_wide(rng, w, fmt, EW, WIDE_PER_ROW[fmt])
    if c.transpose:
        w = np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])    # as the forward weight [O = K, C = M, k, k]
    q = 2.0 ** (ea + EW)
    Ho, Wo = -(-c.H // c.stride), -(-c.W // c.stride)
    bias = rng.integers(-64, 65, c.M) * q * 8
    residual = rng.integers(-16, 17, (c.B, c.M, Ho, Wo)) * 2.0 ** ea
    gate = rng.integers(-1, 2, (c.B, c.M, Ho, Wo)).astype(np.float64)          # a third each: masked by sign, by zero, kept
    return Lattice(_f32(x), _f32(w), q, _f32(bias), _f32(residual), _f32(gate))


def fwd_op(c):
    k = 3 if c.taps == 9 else 1
    return op_grad_input(k, 1, c.H, c.W) if c.transpose else op_forward(k, c.stride)


def epilogue(conv, bias=None, residual=None, relu=False, gate=None):
    """[gate > 0] * [relu](conv + bias[m] + residual) in float64, zeros as +0"""
    v = np.asarray(conv, np.float64)
    if bias is not None:
        v = v + np.asarray(bias, np.float64).reshape(1, -1, 1, 1)
    if residual is not None:
        v = v + np.asarray(residual, np.float64)
    if relu:
        v = np.maximum(v, 0.0)
    if gate is not None:
        v = np.where(np.asarray(gate) > 0, v, 0.0)
    return v + 0.0


@functools.lru_cache(maxsize=4)
def s2gi_lattice(B, C, O, Hin, Win):
    rng = _rng('s2gi', B, C, O, Hin, Win)
    H, W = (Hin + 1) // 2, (Win + 1) // 2
    gy = _sprinkle(rng, _small(rng, (B, O, H, W), EG), BF16, EG, WIDE_DENSITY)
    w = _rows_wide(rng, _small(rng, (C, O, 3, 3), EW), BF16, EW, WIDE_PER_ROW[BF16]).transpose(1, 0, 2, 3)
    return Lattice(_f32(gy), _f32(np.ascontiguousarray(w)), 2.0 ** (EG + EW), None, None, None)


@functools.lru_cache(maxsize=4)
def stem_lattice(B, H, W, fmt):
    rng = _rng('stem', B, H, W, fmt)
    x = _sprinkle(rng, _small(rng, (B, 3, H, W), EA), fmt, EA, WIDE_DENSITY)
    w = _rows_wide(rng, _small(rng, (64, 3, 7, 7), EW), fmt, EW, WIDE_PER_ROW[fmt])
    return Lattice(_f32(x), _f32(w), 2.0 ** (EA + EW), None, None, None)


GwLattice = collections.namedtuple('GwLattice', 'gy x q w s mean var bn_partial')


def gw_geometry(c):
    """(k, stride, Ho, Wo) of a weight-gradient case; 1x1 cases are [.., 1, pixel count]"""
    if c.route == 's2':
        return 3, 2, (c.H + 1) // 2, (c.W + 1) // 2
    return (3 if c.route == '3x3' else 1), 1, c.H, c.W


def gw_op(c):
    k, stride, _, _ = gw_geometry(c)
    return op_grad_weight(k, stride, c.C)


@functools.lru_cache(maxsize=4)
def gw_lattice(name):
    """grad_y [B, O, Ho, Wo] at gradient magnitude with a few wide values per channel, x [B, C, H, W]; for the folded closers the
    weight w, fold scales s (powers of two, one row 0: a zero-initialised gamma), mean, var and bn_partial [O, P] (integers x 2^EG)"""
    c = GW_BY_NAME[name]
    rng = _rng('gw', name)
    k, stride, Ho, Wo = gw_geometry(c)
    x = _sprinkle(rng, _small(rng, (c.B, c.C, c.H, c.W), EA), BF16, EA, WIDE_DENSITY)
    gy = _small(rng, (c.O, c.B, Ho, Wo), EG)
    gy = np.ascontiguousarray(_rows_wide(rng, gy, BF16, EG, WIDE_PER_ROW[BF16]).transpose(1, 0, 2, 3))
    w = _small(rng, (c.O, c.C, k, k), EW)
    s = 2.0 ** rng.integers(-3, 4, c.O)
    s[c.O // 2] = 0.0
    mean = rng.integers(-8, 9, c.O) / 8.0
    var = rng.integers(1, 9, c.O) / 4.0
    bn_partial = rng.integers(-100, 101, (c.O, 5)) * 2.0 ** EG
    return GwLattice(_f32(gy), _f32(x), 2.0 ** (EG + EA), _f32(w), _f32(s), _f32(mean), _f32(var), _f32(bn_partial))


def fold_refs(G, gl, beta, eps):
    """what conv_wsum_fold returns from the summed weight gradient G [O, ...] (float64) and grad_beta: grad_w = s G, grad_gamma =
    (<w, G> - mean grad_beta) / sqrt(var + eps), and the scale of grad_gamma's terms (its bound is counted from them)"""
    O = G.shape[0]
    w, s, mean, var = (np.asarray(t, np.float64) for t in (gl.w, gl.s, gl.mean, gl.var))
    dot = (w.reshape(O, -1) * G.reshape(O, -1)).sum(1)
    rstd = 1.0 / np.sqrt(var + eps)
    scale = (np.abs(w.reshape(O, -1) * G.reshape(O, -1)).sum(1) + np.abs(mean * beta)) * rstd
    return G * s.reshape((O,) + (1,) * (G.ndim - 1)), (dot - mean * beta) * rstd, scale


# mixed scales ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def fwd_mixed(name):
    """activations of order 1 (a transposed case: gradients, image b at 1e-8 x 10^-b, half of them exact zeros as behind a ReLU
    mask), weight rows 0.1 randn x 10^U(-4, 1) per output channel: inside the fp16 envelope's upper end (|w| <= 255)"""
    c = FWD_BY_NAME[name]
    rng = _rng('fwd_mixed', name)
    k = 3 if c.taps == 9 else 1
    x = rng.standard_normal((c.B, c.K, c.H, c.W))
    w = 0.1 * rng.standard_normal((c.M, c.K, k, k)) * 10.0 ** rng.uniform(-4, 1, (c.M, 1, 1, 1))
    if c.transpose:
        x = x * 1e-8 * 10.0 ** -np.arange(c.B).reshape(-1, 1, 1, 1) * (rng.random(x.shape) < 0.5)
        w = 0.1 * rng.standard_normal((c.K, c.M, k, k))
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(w, np.float32)


@functools.lru_cache(maxsize=4)
def s2gi_mixed(B, C, O, Hin, Win):
    rng = _rng('s2gi_mixed', B, C, O, Hin, Win)
    gy = rng.standard_normal((B, O, (Hin + 1) // 2, (Win + 1) // 2))
    gy = gy * 1e-8 * 10.0 ** -np.arange(B).reshape(-1, 1, 1, 1) * (rng.random(gy.shape) < 0.5)
    return np.ascontiguousarray(gy, np.float32), np.ascontiguousarray(0.1 * rng.standard_normal((O, C, 3, 3)), np.float32)


@functools.lru_cache(maxsize=4)
def gw_mixed(name):
    """grad_y channels at 1e-8 x 10^U(-3, 0), half of the elements exact zeros; x of order 1"""
    c = GW_BY_NAME[name]
    rng = _rng('gw_mixed', name)
    _, _, Ho, Wo = gw_geometry(c)
    gy = rng.standard_normal((c.B, c.O, Ho, Wo)) * 1e-8 * 10.0 ** rng.uniform(-3, 0, (1, c.O, 1, 1))
    gy = gy * (rng.random(gy.shape) < 0.5)
    return np.ascontiguousarray(gy, np.float32), np.ascontiguousarray(rng.standard_normal((c.B, c.C, c.H, c.W)), np.float32)


def lattice_ok(terms, q, extra=0.0):
    """the lattice condition of one case: every element's sum of |terms| (+ the epilogue's operands) stays below 2^24 q"""
    return float((np.asarray(terms, np.float64) + extra).max()) < 2.0 ** 24 * q
