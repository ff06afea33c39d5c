"""References of the grouped 3x3 convolutions (csrc/grouped_conv.hip): the three operations in float64 written out over the
groups and taps, operand generators and the case table.  Plain CPU torch / numpy, no GPU.  tests/test_grouped_conv_refs.py pins
the operations to ``F.conv2d(groups=)`` and its autograd in float64; tests/test_gpu_grouped_conv.py holds the kernels to them
through the C ABI, in two tiers:

  exact         operands on an integer lattice (integers of [-3, 3] times a power of two): every term of every result is a multiple
                of one quantum q and sum |terms| < 2^24 q -- also over the B * Ho * Wo pixels of the weight gradient -- so every
                partial sum in every order is an exact float and a correct kernel returns the bits of the float64 result whatever
                its tiling and order;
  accumulation  mixed-scale operands from committed seeds: |got - f64| <= gamma_n * sum |a_i b_i| per element, gamma_n =
                n u / (1 - n u), u = 2^-24, n the number of summands (9 cpg, + 1 with a bias; B Ho Wo for the weight
                gradient): the standard bound of ANY summation order of fp32 products, fused or not.
"""
import collections
import functools
import zlib

import numpy as np
import torch

U = 2.0 ** -24
CPGS = (4, 8, 16, 32)
SMALL_MAPS = ((1, 1), (1, 7), (7, 1), (2, 2), (5, 7), (8, 8))
# one more than a power-of-two tile in each direction; 33 x 65: more than one workgroup of 256 four-pixel strips per plane
# (forward, grad_input); 65 x 129 at B = 3: more than one pixel chunk of the weight gradient (16384 pixels and up)
LARGE_MAPS = ((17, 33), (33, 65), (65, 129))

Case = collections.namedtuple('Case', 'name cpg stride groups B H W')


def out_size(n, stride):
    return (n - 1) // stride + 1


def _cases():
    cases, i = [], 0
    for cpg in CPGS:
        allowed = (1, 3, 32) if cpg in (4, 8) else (1, 3)
        for stride in (1, 2):
            for H, W in SMALL_MAPS:
                groups, B = allowed[i % len(allowed)], (1, 3)[(i // 2) % 2]
                i += 1
                cases.append(Case('c%d_s%d_g%d_b%d_%dx%d' % (cpg, stride, groups, B, H, W), cpg, stride, groups, B, H, W))
            for H, W in LARGE_MAPS:
                B = 3 if (H, W) == (17, 33) or cpg in (4, 32) else 1
                cases.append(Case('c%d_s%d_g3_b%d_%dx%d' % (cpg, stride, B, H, W), cpg, stride, 3, B, H, W))
    return cases


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


# ---------------------------------------------------------------------------------------------- the operations, float64
def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def _taps(Ho, Wo, stride):
    for ky in range(3):
        for kx in range(3):
            yield ky, kx, slice(ky, ky + stride * (Ho - 1) + 1, stride), slice(kx, kx + stride * (Wo - 1) + 1, stride)


def forward(x, w, stride):
    """y [B, C, Ho, Wo] of x [B, C, H, W] and w [C, cpg, 3, 3], padding 1: group by group, tap by tap"""
    x, w = _t(x), _t(w)
    B, C, H, W = x.shape
    cpg = w.shape[1]
    G, Ho, Wo = C // cpg, out_size(H, stride), out_size(W, stride)
    xp = torch.zeros(B, G, cpg, H + 2, W + 2, dtype=torch.float64)
    xp[..., 1:H + 1, 1:W + 1] = x.reshape(B, G, cpg, H, W)
    wg = w.reshape(G, cpg, cpg, 3, 3)          # [group, output channel, input channel, ky, kx]
    y = torch.zeros(B, G, cpg, Ho, Wo, dtype=torch.float64)
    for ky, kx, ys, xs in _taps(Ho, Wo, stride):
        y += torch.einsum('bgchw,goc->bgohw', xp[..., ys, xs], wg[..., ky, kx])
    return y.reshape(B, C, Ho, Wo).numpy()


def grad_input(gy, w, H, W, stride):
    """grad_x [B, C, H, W] from grad_y [B, C, Ho, Wo]: every tap scattered back onto the padded map"""
    gy, w = _t(gy), _t(w)
    B, C, Ho, Wo = gy.shape
    cpg = w.shape[1]
    G = C // cpg
    assert (Ho, Wo) == (out_size(H, stride), out_size(W, stride))
    wg, gyg = w.reshape(G, cpg, cpg, 3, 3), gy.reshape(B, G, cpg, Ho, Wo)
    gxp = torch.zeros(B, G, cpg, H + 2, W + 2, dtype=torch.float64)
    for ky, kx, ys, xs in _taps(Ho, Wo, stride):
        gxp[..., ys, xs] += torch.einsum('bgohw,goc->bgchw', gyg, wg[..., ky, kx])
    return gxp[..., 1:H + 1, 1:W + 1].reshape(B, C, H, W).numpy()


def grad_weight(gy, x, stride, cpg):
    """grad_w [C, cpg, 3, 3] from grad_y [B, C, Ho, Wo] and x [B, C, H, W]: one product over batch and pixels per tap"""
    gy, x = _t(gy), _t(x)
    B, C, H, W = x.shape
    G, Ho, Wo = C // cpg, gy.shape[2], gy.shape[3]
    assert (Ho, Wo) == (out_size(H, stride), out_size(W, stride))
    xp = torch.zeros(B, G, cpg, H + 2, W + 2, dtype=torch.float64)
    xp[..., 1:H + 1, 1:W + 1] = x.reshape(B, G, cpg, H, W)
    gyg = gy.reshape(B, G, cpg, Ho, Wo)
    gw = torch.zeros(G, cpg, cpg, 3, 3, dtype=torch.float64)
    for ky, kx, ys, xs in _taps(Ho, Wo, stride):
        gw[..., ky, kx] = torch.einsum('bgohw,bgchw->goc', gyg, xp[..., ys, xs])
    return gw.reshape(C, cpg, 3, 3).numpy()


def gamma(n):
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------------------------------------- operands
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _f32(a):
    a32 = np.ascontiguousarray(a, np.float32)
    assert (a32.astype(np.float64) == a).all()
    return a32


EA, EW, EG = -3, -6, -20       # exponents of the lattice: activations, weights, gradients

Operands = collections.namedtuple('Operands', 'x w gy bias')


def _shapes(c):
    C = c.groups * c.cpg
    return (c.B, C, c.H, c.W), (C, c.cpg, 3, 3), (c.B, C, out_size(c.H, c.stride), out_size(c.W, c.stride))


@functools.lru_cache(maxsize=None)
def lattice(name):
    """float32 operands that are integers of [-3, 3] times 2^EA (x), 2^EW (w, bias) and 2^EG (grad_y): at most 9 * 32 terms of
    9 quanta per forward / grad_input result and 3 * 65 * 129 terms per weight-gradient result: sum |terms| < 2^24 quanta"""
    c = BY_NAME[name]
    rng = _rng('lattice', name)
    xs, ws, ys = _shapes(c)

    def ints(shape, e):
        return _f32(rng.integers(-3, 4, shape).astype(np.float64) * 2.0 ** e)
    assert 9 * max(9 * c.cpg + 1, ys[0] * ys[2] * ys[3]) < 2 ** 24
    # (the bias on the products' lattice: a multiple of the forward quantum 2^(EA + EW), |bias| <= 3 * 2^6 quanta)
    return Operands(ints(xs, EA), ints(ws, EW), ints(ys, EG), ints((xs[1],), EA + EW + 6))


@functools.lru_cache(maxsize=None)
def mixed(name):
    """mixed-scale operands: normal values whose scale varies over three decades per channel"""
    c = BY_NAME[name]
    rng = _rng('mixed', name)
    xs, ws, ys = _shapes(c)

    def scaled(shape, axis, base):
        s = [1] * len(shape)
        s[axis] = shape[axis]
        return (base * rng.standard_normal(shape) * 10.0 ** rng.uniform(-2, 1, s)).astype(np.float32)
    return Operands(scaled(xs, 1, 1.0), scaled(ws, 0, 0.1), scaled(ys, 1, 1e-3), scaled((xs[1],), 0, 1.0))


@functools.lru_cache(maxsize=None)
def results(name, tier):
    """float64 (forward, grad_input, grad_weight) of the case's operands and, for the mixed tier, the same of their absolute
    values: sum |a_i b_i| per element"""
    c = BY_NAME[name]
    op = lattice(name) if tier == 'lattice' else mixed(name)

    def three(x, w, gy):
        return (forward(x, w, c.stride), grad_input(gy, w, c.H, c.W, c.stride), grad_weight(gy, x, c.stride, c.cpg))
    ref = three(op.x, op.w, op.gy)
    mag = three(np.abs(op.x), np.abs(op.w), np.abs(op.gy)) if tier == 'mixed' else None
    return ref, mag


def summands(c):
    """n of gamma_n per entry point: (forward, grad_input, grad_weight)"""
    return 9 * c.cpg, 9 * c.cpg, c.B * out_size(c.H, c.stride) * out_size(c.W, c.stride)
