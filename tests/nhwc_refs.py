"""References and cases for csrc/conv_nhwc.hip (kgdet_conv1x1_nhwc_residual[_in]) in plain numpy, no GPU:

    out[m][n] = bf16( [relu]( fp32(bf16(S)) + bias[n] + res[m][n] ) ),   S = sum_k a[m][k] w[n][k],
    a = bf16(relu(fp32(x) + in_bias[k])) with in_bias, a = x without.

Exact tier.  Every operand sits on a lattice of q = 2^-15 and every partial sum of every element stays below 2^24 q, so each
addition a correct kernel can make -- in any k order, any tiling, float32 or wider -- is exact and the three roundings to bf16 are
the only inexact steps: the kernel must return the reference's bits.  The reference itself makes the sums in float32 (exact for the
same reason; tests/test_nhwc_refs.py holds it to a float64 evaluation) and rounds with dense_refs.bf16_round_bits.

Mixed-scale tier.  Normal-distributed operands; a correct kernel's float32 accumulation is within e = K 2^-23 sum_k |a w| of the
float64 sum S (any order, exact products, a unit roundoff that also covers a truncating adder), and the map from the sum to the
output is monotone: the output must lie in [final(S - e), final(S + e)] element by element.  Where both ends are the same bf16 --
all but the share pinned in MIXED_AMBIGUOUS -- that is bit equality.
"""
import functools
import itertools

import numpy as np

from tests.dense_refs import bf16_round_bits

f32 = np.float32
Q = 2.0 ** -15                      # the lattice's quantum: (x + in_bias rounded to bf16: 2^-9 at the finest) x (w: 2^-6)
X_RANGE, X_UNIT = 3, 2.0 ** -3      # x: integers in [-3, 3] x 2^-3
W_RANGE, W_UNIT = 3, 2.0 ** -6      # w: integers in [-3, 3] x 2^-6
IB_RANGE, IB_UNIT = 600, 2.0 ** -9  # in_bias: integers in [-600, 600] x 2^-9: x + in_bias is exact in float32, 10+ bits wide on a part
BIAS_RANGE = 2 ** 16                # bias: integers up to 2^16 in magnitude x q
RES_RANGE, RES_UNIT = 127, 2.0 ** 8 * Q   # res: bf16 values (integer in [-127, 127]) x 2^8 q

# (K, N, M): the smallest shapes at which each path of the kernel can go wrong
SMALL_CASES = [
    (16, 128, 1),        # one k-step (the tail loop alone); every row but one clamped to M - 1
    (16, 64, 33),        # half channel tile; the second wave holds one live row
    (80, 256, 127),      # 4 + 1 k-steps; two column tiles (blockIdx % n_ctiles); either side of the 128-row tile
    (80, 256, 129),
    (112, 128, 96),      # 4 + 3 k-steps
    (256, 128, 255),     # the eight-wave variant, either side of its 256-row tile
    (256, 128, 257),
    (384, 128, 300),     # eight waves at their largest LDS
    (400, 128, 130),     # the first K back on four waves; 24 + 1 k-steps
    (512, 128, 200),     # 128 KiB weight tile
]
LARGE_CASES = [
    (16, 128, 768 * 128 + 1),     # persistent loop: workgroup 0 makes a second trip, and that trip is the one-pixel ragged tile
    (256, 128, 768 * 256 + 1),    # the same on eight waves
    (512, 256, 128 * 128 + 5),    # the K > 384 grid cap (256 / n_ctiles workgroups per column tile) looping
]
EXACT_CASES = SMALL_CASES + LARGE_CASES
COMBOS = list(itertools.product((0, 1), repeat=3))       # (relu, in_bias given, residual given): the eight instantiations per wave count
REFUSED = [(24, 128), (528, 128), (16, 192), (16, 32)]   # (K, N) the ABI turns down with KGDET_E_SHAPE

DEFECTS = ('product_not_rounded', 'bias_of_next_channel', 'relu_before_residual', 'last_kstep_dropped', 'in_bias_without_relu',
           'halves_swapped')


def case_id(case):
    return 'K%d-N%d-M%d' % tuple(case)


def combo_id(combo):
    return 'relu%d-in%d-res%d' % tuple(combo)


def defect_applies(defect, case, combo):
    K, N, M = case
    relu, in_epi, with_res = combo
    if defect == 'relu_before_residual':
        return bool(relu and with_res)
    if defect == 'in_bias_without_relu':
        return bool(in_epi)
    if defect == 'halves_swapped':
        return N % 128 == 0       # (N = 64: one half exists)
    return True


def bf16_bits(v):
    """the 16-bit patterns of float32 values that are bf16 already"""
    u = np.ascontiguousarray(v, f32).view(np.uint32)
    assert not (u & 0xffff).any(), 'not bf16 values'
    return (u >> 16).astype(np.uint16)


# ---------------------------------------------------------------------------------------------- exact tier
def worst_case_magnitude(K):
    """an upper bound of sum_k |a w| + |bias| + |res| over ANY draw of the lattice inputs, in units of q"""
    a_max = float(bf16_round_bits(f32(X_RANGE * X_UNIT + IB_RANGE * IB_UNIT)).reshape(-1)[0])
    return (K * a_max * W_RANGE * W_UNIT + BIAS_RANGE * Q + RES_RANGE * RES_UNIT) / Q


@functools.lru_cache(maxsize=2)
def exact_inputs(case):
    """dict of float32 arrays: x0 [M, K], in_bias [K], w [N, K], bias [N], res [M, N] (read-only; shared between the tests)"""
    K, N, M = case
    rng = np.random.default_rng([K, N, M, 20])
    inp = dict(
        x0=rng.integers(-X_RANGE, X_RANGE + 1, (M, K), dtype=np.int8).astype(f32) * f32(X_UNIT),
        in_bias=rng.integers(-IB_RANGE, IB_RANGE + 1, K).astype(f32) * f32(IB_UNIT),
        w=rng.integers(-W_RANGE, W_RANGE + 1, (N, K)).astype(f32) * f32(W_UNIT),
        bias=rng.integers(-BIAS_RANGE, BIAS_RANGE + 1, N).astype(f32) * f32(Q),
        res=rng.integers(-RES_RANGE, RES_RANGE + 1, (M, N), dtype=np.int8).astype(f32) * f32(RES_UNIT))
    for v in inp.values():
        v.setflags(write=False)
    return inp


def activation(inp, in_epi, rows=slice(None)):
    """the x the kernel is handed.  With in_bias: x0, the coarse lattice, so that x0 + in_bias is exact in float32 and needs its
    rounding.  Without: bf16(x0 + in_bias), signed values of full bf16 width on the 2^-9 lattice -- x0 itself has two significant
    bits and its products with w never reach the ninth bit at small K, so bf16(S) would be S and the product's rounding invisible."""
    x0 = inp['x0'][rows]
    return x0 if in_epi else bf16_round_bits(x0 + inp['in_bias'])


def exact_reference(case, combo, defect=None, rows=slice(None), dtype=f32):
    """dict(out, and the values in front of each rounding: pre_a / a, S / Sr, f) of rows `rows`; `defect`: one of DEFECTS, the
    deliberately wrong kernels tests/test_nhwc_refs.py holds the inputs' discrimination to"""
    K, N, M = case
    relu, in_epi, with_res = combo
    inp = exact_inputs(case)
    x = activation(inp, in_epi, rows).astype(dtype)
    if in_epi:
        pre_a = x + inp['in_bias'].astype(dtype)
        if defect != 'in_bias_without_relu':
            pre_a = np.maximum(pre_a, 0)
        a = bf16_round_bits(pre_a).astype(dtype)
    else:
        pre_a = a = x
    w = inp['w'].astype(dtype)
    ak, wk = (a[:, :K - 16], w[:, :K - 16]) if defect == 'last_kstep_dropped' else (a, w)
    S = ak @ wk.T + dtype(0)                                       # (+ 0: a zero sum is +0)
    Sr = S if defect == 'product_not_rounded' else bf16_round_bits(S).astype(dtype)
    bias = inp['bias'].astype(dtype)
    if defect == 'bias_of_next_channel':
        bias = np.roll(bias, -1)
    f = Sr + bias
    res = inp['res'][rows].astype(dtype) if with_res else None
    if defect == 'relu_before_residual':
        f = np.maximum(f, 0) + res
    else:
        if with_res:
            f = f + res
        if relu:
            f = np.maximum(f, 0)
    out = bf16_round_bits(f)
    if defect == 'halves_swapped':
        out = np.ascontiguousarray(out.reshape(-1, N // 128, 2, 64)[:, :, ::-1]).reshape(-1, N)
    return dict(out=out, pre_a=pre_a, a=a, S=S, Sr=Sr, f=f)


def exact_headroom(case, combo, rows=slice(None)):
    """max over the elements of sum_k |a w| + |bias| + |res|, in units of q (the lattice condition: < 2^24)"""
    inp = exact_inputs(case)
    r = exact_reference(case, combo, rows=rows, dtype=np.float64)
    mag = np.abs(r['a']) @ np.abs(inp['w'].astype(np.float64)).T + np.abs(inp['bias'].astype(np.float64))
    if combo[2]:
        mag = mag + np.abs(inp['res'][rows])
    return float(mag.max()) / Q


# ---------------------------------------------------------------------------------------------- mixed-scale tier
MIXED_K = (16, 64, 128, 256, 512)
MIXED_M, MIXED_N = 300, 128
MIXED_CAP = 0.30
# The share of elements whose two interval ends differ (mixed_interval()['ambiguous']), as measured on the CPU with these seeds; every
# element outside it is held bit-exact.  tests/test_nhwc_refs.py recomputes each and holds it to its entry and to MIXED_CAP.
# Key: (K, (relu, in_bias given, residual given)).  It grows with K (e grows as K^1.5 against the output's spacing) and halves with
# the ReLU (half the outputs are 0 at both ends).  K = 512 without the ReLU is beyond the cap (0.32 .. 0.47): those four tell too
# little and are not in MIXED_CASES; K = 512 is run on the four ReLU instantiations.
# On the MI355X every element of every case run lay inside its interval (no excess over e to record).
MIXED_AMBIGUOUS = {
    (16, (0, 0, 0)): 0.0012, (16, (0, 0, 1)): 0.0010, (16, (0, 1, 0)): 0.0006, (16, (0, 1, 1)): 0.0007, (16, (1, 0, 0)): 0.0004, (16, (1, 0, 1)): 0.0003, (16, (1, 1, 0)): 0.0003, (16, (1, 1, 1)): 0.0003,
    (64, (0, 0, 0)): 0.0159, (64, (0, 0, 1)): 0.0148, (64, (0, 1, 0)): 0.0112, (64, (0, 1, 1)): 0.0099, (64, (1, 0, 0)): 0.0090, (64, (1, 0, 1)): 0.0076, (64, (1, 1, 0)): 0.0059, (64, (1, 1, 1)): 0.0051,
    (128, (0, 0, 0)): 0.0563, (128, (0, 0, 1)): 0.0466, (128, (0, 1, 0)): 0.0445, (128, (0, 1, 1)): 0.0383, (128, (1, 0, 0)): 0.0282, (128, (1, 0, 1)): 0.0225, (128, (1, 1, 0)): 0.0232, (128, (1, 1, 1)): 0.0195,
    (256, (0, 0, 0)): 0.1815, (256, (0, 0, 1)): 0.1560, (256, (0, 1, 0)): 0.1414, (256, (0, 1, 1)): 0.1198, (256, (1, 0, 0)): 0.0928, (256, (1, 0, 1)): 0.0794, (256, (1, 1, 0)): 0.0715, (256, (1, 1, 1)): 0.0609,
    (512, (0, 0, 0)): 0.4650, (512, (0, 0, 1)): 0.4279, (512, (0, 1, 0)): 0.3480, (512, (0, 1, 1)): 0.3171, (512, (1, 0, 0)): 0.2324, (512, (1, 0, 1)): 0.2154, (512, (1, 1, 0)): 0.1838, (512, (1, 1, 1)): 0.1673,
}
MIXED_CASES = [(K, c) for K in MIXED_K for c in COMBOS if MIXED_AMBIGUOUS[(K, c)] < MIXED_CAP]


@functools.lru_cache(maxsize=2)
def mixed_inputs(K):
    rng = np.random.default_rng([K, 21])
    inp = dict(x=bf16_round_bits(rng.standard_normal((MIXED_M, K)).astype(f32)),
               in_bias=rng.standard_normal(K).astype(f32),
               w=bf16_round_bits((0.1 * rng.standard_normal((MIXED_N, K))).astype(f32)),
               bias=rng.standard_normal(MIXED_N).astype(f32),
               res=bf16_round_bits(rng.standard_normal((MIXED_M, MIXED_N)).astype(f32)))
    for v in inp.values():
        v.setflags(write=False)
    return inp


def mixed_final(s, inp, combo):
    """the kernel's map from the accumulated sum (float64 here) to the output, its float32 additions in the kernel's order;
    monotone non-decreasing in s"""
    relu, in_epi, with_res = combo
    f = bf16_round_bits(s.astype(f32)) + inp['bias']
    if with_res:
        f = f + inp['res']
    if relu:
        f = np.maximum(f, f32(0))
    return bf16_round_bits(f)


@functools.lru_cache(maxsize=None)
def mixed_interval(K, combo):
    """dict(lo, hi: float32 arrays of bf16 values [M, N]; ambiguous: the share of elements with lo != hi)"""
    relu, in_epi, with_res = combo
    inp = mixed_inputs(K)
    a = bf16_round_bits(np.maximum(inp['x'] + inp['in_bias'], f32(0))) if in_epi else inp['x']
    a64, w64 = a.astype(np.float64), inp['w'].astype(np.float64)
    S = a64 @ w64.T
    e = K * 2.0 ** -23 * (np.abs(a64) @ np.abs(w64).T)
    lo, hi = mixed_final(S - e, inp, combo), mixed_final(S + e, inp, combo)
    assert (lo <= hi).all()
    return dict(lo=lo, hi=hi, ambiguous=float((bf16_bits(lo) != bf16_bits(hi)).mean()))
