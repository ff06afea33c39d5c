"""Deformable convolutions with narrow, numerous weight groups (plain numpy, no GPU): the shapes a ResNeXt block's
``dcn['groups']`` reaches, on the smallest maps that still cross each routing decision of csrc/dcn_api.hip.

A case is ``(N, C, H, W, O, k, stride, pad, dil, groups, dg)`` as in tests/test_gpu_dcn.py.  csrc/dcn_api.hip routes every call from
``Cg = C / groups``, ``Og = O / groups``, the channel runs (maximal runs of input channels inside one weight group AND one
deformable group), the input map's H * W and the deformable groups; `facts` restates those definitions in Python and
tests/test_dcn_group_cases.py holds them -- and the constants below -- to the table and to the kernel sources.

Inputs follow tests/test_gpu_dcn.py::_make: a seeded ``default_rng``, offsets of scale 2, weights of scale 0.05, a uniform mask and
a ``linspace`` bias.
"""
import functools

import numpy as np

import oracle

# csrc/dcn_common.h, csrc/dcn_api.hip (tests/test_dcn_group_cases.py reads them back from the sources)
CHUNK = 16                 # kChunk: reduction elements per stage; Cg_pad = align_up(Cg, 16)
TILE_M = 256               # kTileM: Og_pad = align_up(Og, 256)
MAX_RUNS = 8               # kMaxFwdGroup: more channel runs turn the plane grad_input kernel off
PLANE_MAX_HW = 1344        # kPlaneMaxHW: the LDS-plane kernels
EXACT_MAX_HW = 17 * 64     # plan_bwd_lds: the 'exact' gather backward
LARGE_OG_MULTIPLE = 16     # dcn_bwd_large takes a run only if Og % 16 == 0 and (K * Cg) % 2 == 0

SEED = 5

# ResNeXt classes (dg = 1): every entry point must compute these
RESNEXT = [
    # N, C, H, W, O, k, stride, pad, dil, groups, dg
    ('8x4', (2, 32, 9, 11, 32, 3, 1, 1, 1, 8, 1)),             # the small net of tests/resnext_cases.py: exactly MAX_RUNS runs
    ('8x4-stride2', (2, 32, 13, 9, 32, 3, 2, 1, 1, 8, 1)),     # the same at stride 2, odd map
    ('9x4', (1, 36, 9, 11, 36, 3, 1, 1, 1, 9, 1)),             # one run past the limit
    ('32x4', (1, 128, 9, 11, 128, 3, 1, 1, 1, 32, 1)),         # X101 layer1
    ('32x8-stride2', (1, 256, 9, 11, 256, 3, 2, 1, 1, 32, 1)),
    ('32x16', (1, 512, 7, 6, 512, 3, 1, 1, 1, 32, 1)),         # one whole reduction chunk per group
    ('32x32', (1, 1024, 5, 6, 1024, 3, 1, 1, 1, 32, 1)),
    ('8x1-depthwise', (1, 8, 7, 6, 8, 3, 1, 1, 1, 8, 1)),      # Cg = Og = 1, K * Cg odd
    ('8x2-Og6', (1, 16, 7, 6, 48, 3, 1, 1, 1, 8, 1)),          # Og != Cg, neither a multiple of 4
    ('8x6-Og3', (1, 48, 7, 6, 24, 3, 1, 1, 1, 8, 1)),          # Cg = 6: no channel quad
    ('8x4-5x5', (1, 32, 9, 11, 32, 5, 1, 2, 1, 8, 1)),         # 25 taps, the last tap group padded
    ('8x4-1200px', (1, 32, 30, 40, 32, 3, 1, 1, 1, 8, 1)),     # above plan_bwd_lds' 1088, below 1344
    ('8x4-1368px', (1, 32, 38, 36, 32, 3, 1, 1, 1, 8, 1)),     # dcn_bwd_large per run, Og % 16 != 0: the padded path, 8 groups
    ('32x4-1368px', (1, 128, 38, 36, 128, 3, 1, 1, 1, 32, 1)),  # the same with 32 groups
    ('8x1-1368px', (1, 8, 38, 36, 8, 3, 1, 1, 1, 8, 1)),       # input channels padded too, grad_input sliced back
]
# deformable groups against narrow weight groups: every entry point computes or refuses (NotImplementedError)
MIXED = [
    ('8x4-dg8', (2, 32, 9, 11, 32, 3, 1, 1, 1, 8, 8)),         # dg == groups, cpdg = 4
    ('8x8-dg2', (2, 64, 9, 11, 64, 3, 1, 1, 1, 8, 2)),         # one deformable group spans four weight groups
    ('2x32-dg8', (2, 64, 9, 11, 64, 3, 1, 1, 1, 2, 8)),        # one weight group spans four deformable groups of 8 channels
]
NAMES = {case: name for name, case in RESNEXT + MIXED}
BY_NAME = {name: case for name, case in RESNEXT + MIXED}
RESNEXT_CASES = [case for _, case in RESNEXT]
MIXED_CASES = [case for _, case in MIXED]
CASES = RESNEXT_CASES + MIXED_CASES
assert len(NAMES) == len(BY_NAME) == len(CASES)

# the cases of the tests that take a subset
GUARDED = [BY_NAME[n] for n in ('8x4', '32x4', '8x1-depthwise', '8x6-Og3', '32x4-1368px')]
ISOLATED = [BY_NAME[n] for n in ('8x4', '32x4')]
REPEATED = [BY_NAME[n] for n in ('8x4', '32x4', '32x4-1368px')]


def case_id(case):
    return '%s-%s' % (NAMES[case], 'x'.join(str(v) for v in case))


def output_size(case):
    N, C, H, W, O, k, s, p, d, g, dg = case
    return oracle.conv_output_size(H, W, k, k, s, p, d)


def channel_runs(case):
    """[(c0, c1, weight group, deformable group)]: channel_runs of csrc/dcn_api.hip"""
    N, C, H, W, O, k, s, p, d, g, dg = case
    Cg, cpdg = C // g, C // dg
    runs, c0 = [], 0
    while c0 < C:
        gi, di = c0 // Cg, c0 // cpdg
        c1 = min((gi + 1) * Cg, (di + 1) * cpdg)
        runs.append((c0, c1, gi, di))
        c0 = c1
    return runs


def map_class(case):
    """'lds' (H * W <= 1088: every kernel), 'plane' (<= 1344: the plane kernels, 'exact' on the large-map path) or 'large'"""
    hw = case[2] * case[3]
    return 'lds' if hw <= EXACT_MAX_HW else 'plane' if hw <= PLANE_MAX_HW else 'large'


def _align_up(v, a):
    return -(-v // a) * a


def facts(case):
    """what csrc/dcn_api.hip derives from a shape before it picks a route"""
    N, C, H, W, O, k, s, p, d, g, dg = case
    Cg, Og, K = C // g, O // g, k * k
    runs = channel_runs(case)
    large = map_class(case) == 'large'
    # backward_input of a ResNeXt class (dg == 1, groups > 1; plane_bwd_offset_ok is false for all of them, in both arithmetics):
    # dcn_bwd_input_gather up to plan_bwd_lds' limit, dcn_bwd_large per channel run beyond it -- on the zero-padded groups of
    # dcn._backward_input_padded where a run is not eligible (dcn_bwd_large_ok)
    route = None
    if dg == 1 and g > 1:
        eligible = Og % LARGE_OG_MULTIPLE == 0 and (K * Cg) % 2 == 0
        route = 'gather' if H * W <= EXACT_MAX_HW else 'large' if eligible else 'large-padded'
    return dict(Cg=Cg, Og=Og, K=K, cpdg=C // dg, n_runs=len(runs), map_class=map_class(case),
                Cg_pad=_align_up(Cg, CHUNK), Og_pad=_align_up(Og, TILE_M), Og_pad16=_align_up(Og, CHUNK),
                taps_times_channels_odd=(K * Cg) % 2 == 1,
                plane_grad_input=not large and len(runs) <= MAX_RUNS,
                backward_input_route=route,
                exact_slices=g * -(-Cg // 32))


def make(case, v2, seed=SEED):
    """float32 x, off, w, go, mask (v2), bias (v2) in the draw order of tests/test_gpu_dcn.py::_make"""
    N, C, H, W, O, k, s, p, d, g, dg = case
    rng = np.random.default_rng(seed)
    Ho, Wo = output_size(case)
    x = rng.normal(size=(N, C, H, W)).astype(np.float32)
    off = (rng.normal(size=(N, dg * 2 * k * k, Ho, Wo)) * 2.0).astype(np.float32)
    w = (rng.normal(size=(O, C // g, k, k)) * 0.05).astype(np.float32)
    go = rng.normal(size=(N, O, Ho, Wo)).astype(np.float32)
    mask = rng.uniform(size=(N, dg * k * k, Ho, Wo)).astype(np.float32) if v2 else None
    bias = np.linspace(-1, 1, O).astype(np.float32) if v2 else None
    return dict(x=x, off=off, w=w, go=go, mask=mask, bias=bias)


def compute(inputs, case, v2, dtype=np.float64):
    """the oracle's forward and backward of float32 `inputs` in `dtype`: dict(y, grad_input, grad_offset, grad_weight[, grad_mask,
    grad_bias])"""
    N, C, H, W, O, k, s, p, d, g, dg = case
    c = lambda a: None if a is None else a.astype(dtype)
    x, off, w, go, mask, bias = (c(inputs[n]) for n in ('x', 'off', 'w', 'go', 'mask', 'bias'))
    res = dict(y=oracle.deform_conv_forward(x, off, w, s, p, d, g, dg, mask=mask, bias=bias))
    res.update(oracle.deform_conv_backward(x, off, w, go, s, p, d, g, dg, mask=mask, with_bias=v2))
    return res


def _freeze(res):
    for a in res.values():
        if a is not None:
            a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def reference(case, v2, dtype=np.float64):
    """inputs (float32) and the oracle's results in `dtype` of (case, v1 / v2): computed once, shared, read-only"""
    res = make(case, v2)
    res.update(compute(res, case, v2, dtype))
    return _freeze(res)


def grads(v2):
    return ('grad_input', 'grad_offset', 'grad_weight') + (('grad_mask', 'grad_bias') if v2 else ())
