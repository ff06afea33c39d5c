"""Deformable-convolution inputs that sit ON the edges of the sampling rule (plain numpy, no GPU).

Every deformable kernel of csrc/dcn_*.hip restates one rule of the reference: a tap is alive inside the open box
(-1, H) x (-1, W), each of the four bilinear corners has its own validity test, and the slope for grad_offset comes from the floor
cell whatever the weights are.  Random offsets land on the lattice, on -1, on L-1 or on L with probability zero, so `>` against `>=`
at those values cannot be told apart by them.  The generators here put a chosen share of the (image, deformable group, tap, output
pixel) sites exactly onto such positions.

A case is ``(N, C, H, W, O, k, stride, pad, dil, groups, dg)`` as in tests/test_gpu_dcn.py.

Exactness: targets are dyadic rationals of small magnitude (multiples of 2**-10 below 64) and the remaining sites take multiples of
1/8, so ``offset = target - base`` and ``base + offset`` are exact in float32: the float32 kernels and the float64 oracle see the SAME
position, and no element needs a "rounded onto the other side of a cell boundary" allowance.  The huge targets (1e4, 3e9) round,
but stay far outside the map either way.

NaN and infinite offsets are left out on purpose: the reference converts ``floor(NaN)`` to int in its backward pass, which is
undefined behaviour, so there is no reference value to hold the kernels to.
"""
import numpy as np

import oracle

E = 2.0 ** -10

# the shapes of tests/test_dcn_edge_cases.py and tests/test_gpu_dcn_edges.py, and what each is there for
CASES = [
    # N, C, H, W, O, k, stride, pad, dil, groups, dg
    (2, 16, 6, 7, 32, 3, 1, 1, 1, 1, 1),      # plane kernels; O % 32 == 0, but one chunk per tap: no static schedule, dcn_bwd_offset_plane<2>
    (2, 16, 6, 7, 16, 3, 1, 1, 1, 1, 1),      # O = 16: grad_offset on dcn_bwd_offset_plane<2>; masked: its v2 variant
    (2, 6, 6, 7, 10, 3, 1, 1, 1, 1, 1),       # channel counts inside one 16-chunk, padded rows
    (2, 16, 5, 2, 16, 3, 1, 1, 1, 1, 1),      # W == 2: both end branches of make_tap_pair on one column pair
    (2, 16, 1, 9, 16, 3, 1, 1, 1, 1, 1),      # H == 1: the high row is never valid
    (1, 32, 9, 5, 16, 3, 2, 1, 2, 2, 2),      # stride 2, dilation 2, two weight groups x two deformable groups of 16 channels
    (1, 16, 7, 6, 16, 5, 1, 2, 1, 1, 1),      # 5x5 taps (K = 25)
    (1, 16, 7, 6, 16, 7, 1, 3, 1, 1, 1),      # 7x7 taps (K = 49)
    (1, 16, 38, 36, 16, 3, 1, 1, 1, 1, 1),    # 1 368 pixels, above the LDS plane (1 344): gather forward, large-map backward
    (1, 32, 38, 36, 32, 3, 1, 1, 1, 2, 2),    # the same with weight groups and deformable groups
    # two chunks per tap, O % 32 == 0: the fewest channels at which plan_static_ranges gives grad_offset its static schedule (two
    # tiles of 18 stages on two workgroups; with 16 channels the two tiles meet ONE workgroup), i.e. the tap-pair kernel
    (2, 32, 6, 7, 32, 3, 1, 1, 1, 1, 1),      # unmasked: grad_offset on dcn_bwd_offset_pair, blocked input copy or registers
]
SMALL_CASES = [c for c in CASES if c[2] * c[3] <= 1344]
LARGE_CASES = [c for c in CASES if c[2] * c[3] > 1344]

CLASSES = ('on_-1', 'in_(-1,0)', 'lattice', 'inside_off_lattice', 'in_(L-1,L)', 'on_L', 'outside', 'beyond_int32')


def case_id(case):
    return 'x'.join(str(v) for v in case)


def output_size(case):
    N, C, H, W, O, k, s, p, d, g, dg = case
    return oracle.conv_output_size(H, W, k, k, s, p, d)


def palette(L):
    """the target positions of one axis of length L (float64; every one but the last four is exact in float32)"""
    mid, third = (L - 1) // 2, (L - 1) // 3
    vals = [-1, -1 + E, -0.5, 0, 0.25, 1, L - 2, L - 1 - E, L - 1, L - 1 + E, L - 0.5, L - E, L, L + 3, -7,
            1e4, -1e4, 3e9, -3e9,
            mid, third, mid + 0.25, third + 0.75]      # two interior lattice points, two interior quarter points
    return np.asarray(vals, np.float64)


def base_grid(case):
    """(base_y, base_x): int arrays [K, Ho, Wo], the undeformed position o * stride - pad + i * dil of every (tap, output pixel)"""
    N, C, H, W, O, k, s, p, d, g, dg = case
    Ho, Wo = output_size(case)
    oy, ox = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing='ij')
    ti, tj = np.divmod(np.arange(k * k), k)
    by = oy[None] * s - p + ti[:, None, None] * d
    bx = ox[None] * s - p + tj[:, None, None] * d
    return by, bx


def edge_offsets(case, seed, edge_share=0.5):
    """float32 offsets [N, dg*2*k*k, Ho, Wo]: a share `edge_share` of the sites samples at palette positions (both axes drawn
    independently), the others at ``round(normal * 2 * 8) / 8`` from the undeformed position"""
    N, C, H, W, O, k, s, p, d, g, dg = case
    Ho, Wo = output_size(case)
    K = k * k
    rng = np.random.default_rng(seed)
    by, bx = base_grid(case)
    sites = (N, dg, K, Ho, Wo)
    edge = rng.random(sites) < edge_share
    out = np.empty((N, dg, K, 2, Ho, Wo), np.float32)
    for axis, (L, base) in enumerate(((H, by), (W, bx))):
        pal = palette(L).astype(np.float32)
        target = pal[rng.integers(0, len(pal), size=sites)]
        on_edge = target - base.astype(np.float32)          # in float32, and exact there (module docstring)
        free = (np.round(rng.standard_normal(sites) * 2 * 8) / 8).astype(np.float32)
        out[:, :, :, axis] = np.where(edge, on_edge, free)
    return np.ascontiguousarray(out.reshape(N, dg * 2 * K, Ho, Wo))


def edge_mask(case, seed):
    """float32 modulation mask [N, dg*k*k, Ho, Wo]: uniform in [0, 1), 20 % of the elements exactly 0 (saturated), 2 % (at least three) exactly 1"""
    N, C, H, W, O, k, s, p, d, g, dg = case
    Ho, Wo = output_size(case)
    rng = np.random.default_rng(seed)
    shape = (N, dg * k * k, Ho, Wo)
    m = rng.random(shape).astype(np.float32).reshape(-1)
    order = rng.permutation(m.size)
    n0, n1 = round(0.2 * m.size), max(3, round(0.02 * m.size))
    m[order[:n0]] = 0.0
    m[order[n0:n0 + n1]] = 1.0
    return m.reshape(shape)


def all_outside(case):
    """every offset is +1e4: no tap of no pixel is alive"""
    N, C, H, W, O, k, s, p, d, g, dg = case
    Ho, Wo = output_size(case)
    return np.full((N, dg * 2 * k * k, Ho, Wo), 1e4, np.float32)


def lattice(case):
    """all-zero offsets: the state init_offset() leaves -- every position on the lattice, fractions exactly 0"""
    return np.zeros_like(all_outside(case))


def positions(case, offset, dtype):
    """(y, x) [N, dg, K, Ho, Wo]: ``base + offset`` evaluated in `dtype`, the way the kernels (float32) / the oracle (float64) do"""
    N, C, H, W, O, k, s, p, d, g, dg = case
    Ho, Wo = output_size(case)
    by, bx = base_grid(case)
    o = offset.reshape(N, dg, k * k, 2, Ho, Wo).astype(dtype)
    return by.astype(dtype) + o[:, :, :, 0], bx.astype(dtype) + o[:, :, :, 1]


def classify_axis(pos, L):
    """{class: number of sites} for the positions of one axis of length L"""
    pos = np.asarray(pos, np.float64)
    whole = pos == np.floor(pos)
    return {
        'on_-1': int((pos == -1).sum()),
        'in_(-1,0)': int(((pos > -1) & (pos < 0)).sum()),
        'lattice': int((whole & (pos >= 0) & (pos <= L - 1)).sum()),
        'inside_off_lattice': int((~whole & (pos > 0) & (pos < L - 1)).sum()),
        'in_(L-1,L)': int(((pos > L - 1) & (pos < L)).sum()),
        'on_L': int((pos == L).sum()),
        'outside': int(((pos < -1) | (pos > L)).sum()),
        'beyond_int32': int((np.abs(pos) > 2.0 ** 31).sum()),
    }


def classify(case, offset):
    """{'y': {class: count}, 'x': {class: count}} of an offset tensor"""
    y, x = positions(case, offset, np.float64)
    return {'y': classify_axis(y, case[2]), 'x': classify_axis(x, case[3])}


def impossible_classes(case):
    """the classes a shape cannot produce, per axis: an axis of length 1 has no open interval (0, L-1)"""
    return {'y': {'inside_off_lattice'} if case[2] <= 1 else set(), 'x': {'inside_off_lattice'} if case[3] <= 1 else set()}


def tensors(case, seed):
    """x, weight, grad_out, bias (float32) of a case -- what tests/test_gpu_dcn.py draws, from one seed"""
    N, C, H, W, O, k, s, p, d, g, dg = case
    Ho, Wo = output_size(case)
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, C, H, W)).astype(np.float32)
    w = (rng.normal(size=(O, C // g, k, k)) * 0.05).astype(np.float32)
    go = rng.normal(size=(N, O, Ho, Wo)).astype(np.float32)
    bias = np.linspace(-1, 1, O).astype(np.float32)
    return x, w, go, bias


OFFSET_KINDS = {
    'edge': lambda case, seed: edge_offsets(case, seed),
    'lattice': lambda case, seed: lattice(case),
    'outside': lambda case, seed: all_outside(case),
}


def reference(case, kind, v2, seed, dtype=np.float64):
    """the oracle's forward and backward of (case, offset kind, v1 / v2) in `dtype`:
    dict(x, off, w, go, mask, bias [float32 inputs], y, grad_input, grad_offset, grad_weight[, grad_mask, grad_bias])"""
    N, C, H, W, O, k, s, p, d, g, dg = case
    x, w, go, bias = tensors(case, seed)
    off = OFFSET_KINDS[kind](case, seed + 100)
    mask = edge_mask(case, seed + 200) if v2 else None
    c = lambda a: None if a is None else a.astype(dtype)
    res = dict(x=x, off=off, w=w, go=go, mask=mask, bias=bias if v2 else None)
    res['y'] = oracle.deform_conv_forward(c(x), c(off), c(w), s, p, d, g, dg, mask=c(mask), bias=c(bias) if v2 else None)
    res.update(oracle.deform_conv_backward(c(x), c(off), c(w), c(go), s, p, d, g, dg, mask=c(mask), with_bias=v2))
    for a in res.values():
        if a is not None:
            a.setflags(write=False)
    return res
