"""float64 references of the small kernels between the convolutions of every step (csrc/moment.hip, glue.hip, epilogue.hip,
bn_act.hip), their float32 / bf16 restatements, and the rounding bounds the kernels are held to.

Plain numpy / CPU torch, no GPU.  tests/test_pointwise_refs.py pins the references to torch's own CPU operators and the
restatements to their bounds; tests/test_gpu_pointwise_kernels.py holds the kernels to them through the C ABI.
Where a kernel promises bit-identity (glue.hip compiles with contraction off; the epilogues add, add, clamp and round once) the
restatement performs the kernel's roundings one at a time and the bar is equality of bits.  Otherwise the bar is a bound
counted from the kernel's own expression, U = 2^-24 per fp32 rounding -- except for the moment box, whose bar is measured
(moment_bar).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
f32 = np.float32


def f64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.float64)


# ---------------------------------------------------------------------------------------------- moment bounding box
MOMENT_N = [2, 3, 9, 15, 16, 17, 25, 83]
MOMENT_SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (2, 1050), (3, 4200), (2, 16800)]
MOMENT_REGIMES = ['zero', 'offset']


def moment_shapes(n):
    """the (B, HW) run with n points: all of them"""
    return list(MOMENT_SHAPES)


MOMENT_EQUAL = {'zero': 37.3, 'offset': 4001.7}      # the value of the location whose points all coincide


def moment_inputs(B, n, HW, regime):
    """px, py [B, n, HW] float32 (the x and the y of the n points of every location), transfer [2], grad_bbox [B, 4, HW].
    'zero': 3 randn, the data of every earlier test.  'offset': a common offset of +-2048 .. 4096 per location and coordinate plus
    a spread of 1e-2 .. 1e-1 -- the mean's own rounding error is a sizeable part of the spread there, what the residual pass exists for.  With more than one location, location 0 of image 0
    holds n equal points (std == 0)."""
    rng = np.random.default_rng(1000 * n + 10 * HW + B + (5 if regime == 'offset' else 0))
    if regime == 'zero':
        px, py = (3 * rng.standard_normal((B, n, HW)) for _ in range(2))
    else:
        def one():
            off = 4096.0 * rng.uniform(0.5, 1.0, (B, 1, HW)) * rng.choice([-1.0, 1.0], (B, 1, HW))
            return off + 10.0 ** rng.uniform(-2, -1, (B, 1, HW)) * rng.standard_normal((B, n, HW))
        px, py = one(), one()
    px, py = px.astype(f32), py.astype(f32)
    if B * HW > 1:
        px[0, :, 0] = py[0, :, 0] = f32(MOMENT_EQUAL[regime])
    transfer = np.array([0.3, -0.2], f32)
    gb = rng.standard_normal((B, 4, HW)).astype(f32)
    return px, py, transfer, gb


def moment_pack(px, py, y_first):
    """[B, 2 n, HW], channel = (point, y | x) when y_first else (point, x | y)"""
    B, n, HW = px.shape
    pair = (py, px) if y_first else (px, py)
    return np.ascontiguousarray(np.stack(pair, 2).reshape(B, 2 * n, HW))


def moment_unpack(a, y_first):
    B, n2, HW = a.shape
    a = a.reshape(B, n2 // 2, 2, HW)
    return (a[:, :, 1], a[:, :, 0]) if y_first else (a[:, :, 0], a[:, :, 1])


def moment_f64(px, py, transfer, gb):
    """float64: bbox [B, 4, HW] = (mean_x - hw, mean_y - hh, mean_x + hw, mean_y + hh), h. = unbiased std * exp(transfer .);
    gpx, gpy [B, n, HW], gt [2].  At std == 0 the deviation term of the point gradient is taken as 0 (the kernel's choice:
    moment_bbox_backward in include/kgdet_hip.h, and what torch.std's backward fills in; sqrt(var) written out gives NaN).  Also the scales of moment_bar."""
    px, py, t, g = f64(px), f64(py), f64(transfer), f64(gb)
    n = px.shape[1]
    out = {}
    boxes, gts = {}, []
    for k, (v, lo, hi) in enumerate(((px, 0, 2), (py, 1, 3))):
        mean = v.mean(1, keepdims=True)
        d = v - mean
        std = np.sqrt((d * d).sum(1, keepdims=True) / (n - 1))
        e = math.exp(t[k])
        half = std * e
        boxes[lo], boxes[hi] = (mean - half)[:, 0], (mean + half)[:, 0]
        dh = (g[:, hi] - g[:, lo])[:, None]
        mg = (g[:, hi] + g[:, lo])[:, None] / n
        with np.errstate(all='ignore'):
            c = np.where(std > 0, dh * e / ((n - 1) * std), 0.0)
        out['gpx' if k == 0 else 'gpy'] = mg + c * d
        gts.append(float((dh * half).sum()))
        A = np.abs(v).mean(1, keepdims=True)
        out['scale_gpx' if k == 0 else 'scale_gpy'] = np.abs(mg) + np.abs(c) * (np.abs(d) + A)
        out['scale_box%d' % k] = (A + half)[:, 0]
        out['scale_gt%d' % k] = float(np.abs(dh * half).sum())
    out['bbox'] = np.stack([boxes[0], boxes[1], boxes[2], boxes[3]], 1)
    out['scale_bbox'] = np.stack([out['scale_box0'], out['scale_box1'], out['scale_box0'], out['scale_box1']], 1)
    out['gt'] = np.array(gts)
    out['scale_gt'] = np.array([out['scale_gt0'], out['scale_gt1']])
    return out


def _moments_f32(v, residual=True):
    """csrc/moment.hip moments() in serial order, one float32 rounding per operation: the sum, the residual of the mean, the
    squared deviations from the corrected mean (residual=False: the algorithm WITHOUT its second pass, for the CPU check that
    the bar tells the two apart)"""
    n = v.shape[1]
    s = np.zeros_like(v[:, 0])
    for i in range(n):
        s = s + v[:, i]
    mean = s / f32(n)
    s2 = np.zeros_like(s)
    for i in range(n):
        s2 = s2 + (v[:, i] - mean)
    m2 = s2 / f32(n) if residual else f32(0)
    q = np.zeros_like(s)
    for i in range(n):
        d = (v[:, i] - mean) - m2
        q = q + d * d
    return mean, np.sqrt(q / f32(n - 1))


def moment_f32(px, py, transfer, gb, residual=True):
    """the kernels' algorithm in numpy float32, serial order, no fused multiply-add; the transfer gradient as a serial sum over
    the locations"""
    px, py, t, g = (np.asarray(a, f32) for a in (px, py, transfer, gb))
    n = px.shape[1]
    out, boxes, gts = {}, {}, []
    for k, (v, lo, hi) in enumerate(((px, 0, 2), (py, 1, 3))):
        mean, std = _moments_f32(v, residual)
        e = np.exp(t[k])
        half = std * e
        boxes[lo], boxes[hi] = mean - half, mean + half
        dh = g[:, hi] - g[:, lo]
        with np.errstate(all='ignore'):
            c = np.where(std > 0, dh * e / (f32(n - 1) * std), f32(0))
        mg = (g[:, lo] + g[:, hi]) / f32(n)
        out['gpx' if k == 0 else 'gpy'] = mg[:, None] + c[:, None] * (v - mean[:, None])
        terms = (dh * std * e).reshape(-1)
        gts.append(np.cumsum(terms, dtype=f32)[-1])
    out['bbox'] = np.stack([boxes[0], boxes[1], boxes[2], boxes[3]], 1)
    out['gt'] = np.array(gts, f32)
    return out


MOMENT_OUTPUTS = ['bbox', 'gpx', 'gpy', 'gt']


def moment_errors(px, py, transfer, gb, residual=True):
    """max over each output of |float32 restatement - float64| / scale, in units of U.  The scales (moment_f64) are the
    magnitudes an fp32 error is relative to: bbox |v|-mean + half extent; grad_pts |mean term| + |c| (|p - mean| + |v|-mean) --
    the mean's own rounding error, relative to |v|, enters the deviation p - mean --; grad_transfer sum |terms|."""
    ref, r32 = moment_f64(px, py, transfer, gb), moment_f32(px, py, transfer, gb, residual)
    out = {}
    for k in MOMENT_OUTPUTS:
        err, sc = np.abs(r32[k].astype(np.float64) - ref[k]), ref['scale_' + k]
        with np.errstate(all='ignore'):
            out[k] = float(np.max(np.where(err == 0, 0.0, err / (U * sc))))
    return out


@functools.lru_cache(maxsize=None)
def moment_bar(n, regime):
    """The measured tolerance of the moment kernels, per output in units of U * scale: the serial float32 restatement's largest
    error against float64 over every GPU-test input of this n and value regime (moment_shapes; y_first only permutes channels),
    but not less than one rounding of the output, times 4.  The margin covers the kernel's 16-way split of the points and its
    different summation tree (block, butterfly, block order): they change the order of at most n + 16 additions, not the
    algorithm.  Pooling the shapes keeps a one-location input from being judged by the luck of one serial sum."""
    worst = {k: 1.0 for k in MOMENT_OUTPUTS}
    for B, HW in moment_shapes(n):
        e = moment_errors(*moment_inputs(B, n, HW, regime))
        worst = {k: max(worst[k], e[k]) for k in worst}
    return {k: 4.0 * v for k, v in worst.items()}


# ---------------------------------------------------------------------------------------------- glue
def reppts_offsets_f32(reppts, kernel_sizes, gm):
    """the three offset tensors of csrc/glue.hip reppts_offsets_forward in float32, every operation rounded on its own:
    (gm v + (1 - gm) v) - base, base = the regular grid's (y, x) of tap cc / 2, row-major"""
    v = np.asarray(reppts, f32)
    gm = f32(gm)
    outs, first = [], 0
    for k in kernel_sizes:
        cnt, pad = 2 * k * k, (k - 1) // 2
        cc = np.arange(cnt)
        t = cc >> 1
        base = np.where(cc & 1, t % k - pad, t // k - pad).astype(f32)[None, :, None]
        part = v[:, first:first + cnt]
        part = gm * part + (f32(1) - gm) * part
        outs.append((part - base).astype(f32))
        first += cnt
    return outs


def reppts_offsets_grad_f32(grads, kernel_sizes, gm, B, C, HW):
    """grad_reppts [B, C, HW]: gm * grad_k on the slices (None: zeros), exactly 0 beyond them"""
    out, first = np.zeros((B, C, HW), f32), 0
    for g, k in zip(grads, kernel_sizes):
        cnt = 2 * k * k
        if g is not None:
            out[:, first:first + cnt] = f32(gm) * np.asarray(g, f32)
        first += cnt
    return out


def subsample2(x):
    return np.ascontiguousarray(np.asarray(x)[:, ::2, ::2])


def subsample2_grad(gy, H, W, other=None):
    """zero-stuffed grad_y (+ other): at most one addition per element"""
    gx = np.zeros((gy.shape[0], H, W), gy.dtype)
    gx[:, ::2, ::2] = gy
    return gx if other is None else (gx + np.asarray(other, gy.dtype)).astype(gy.dtype)


def pts_from_offsets_f32(pred, centres, stride, y_first):
    """pred [B, 2 n, HW] -> pts [B, HW, 2 n] with (x, y) interleaved: fl(fl(offset * stride) + centre)"""
    p = np.asarray(pred, f32)
    B, C, HW = p.shape
    p = p.reshape(B, C // 2, 2, HW)
    if y_first:
        p = p[:, :, ::-1]
    p = p.transpose(0, 3, 1, 2)                                   # [B, HW, n, (x, y)]
    out = (p * f32(stride)).astype(f32) + np.asarray(centres, f32)[:, :, None, :]
    return np.ascontiguousarray(out.astype(f32).reshape(B, HW, C))


def pts_from_offsets_grad_f32(grad_pts, stride, y_first):
    g = np.asarray(grad_pts, f32)
    B, HW, C = g.shape
    g = g.reshape(B, HW, C // 2, 2)
    if y_first:
        g = g[..., ::-1]
    return np.ascontiguousarray((g.transpose(0, 2, 3, 1) * f32(stride)).astype(f32).reshape(B, C, HW))


# ---------------------------------------------------------------------------------------------- inference epilogues
def bias_act_restated(x, bias, res, relu, channels_last):
    """csrc/epilogue.hip bias_act on CPU torch tensors, x [N, C, HW] (or [N, HW, C]) float32 or bfloat16: x + b, + r, max(., 0)
    each rounded in float32, then ONE round-to-nearest-even to the storage type"""
    v = x.float()
    if bias is not None:
        b = torch.as_tensor(bias, dtype=torch.float32)
        v = v + (b[None, None, :] if channels_last else b[None, :, None])
    else:
        v = v + 0.0
    if res is not None:
        v = v + res.float()
    if relu:
        v = torch.clamp_min(v, 0.0)
    return v.to(x.dtype)


def bias_act_f64(x, bias, res, relu, channels_last):
    v = x.double()
    if bias is not None:
        b = torch.as_tensor(bias, dtype=torch.float64)
        v = v + (b[None, None, :] if channels_last else b[None, :, None])
    if res is not None:
        v = v + res.double()
    return torch.relu(v) if relu else v


def bias_relu_maxpool_restated(x, bias):
    """x [N, H, W, C] -> [N, Ho, Wo, C]: relu(x + b) rounded to the storage type BEFORE the 3x3 / stride 2 / padding 1 maximum"""
    v = x.float()
    if bias is not None:
        v = v + torch.as_tensor(bias, dtype=torch.float32)
    v = torch.clamp_min(v, 0.0).to(x.dtype).float()
    y = F.max_pool2d(v.permute(0, 3, 1, 2), 3, 2, 1)
    return y.permute(0, 2, 3, 1).contiguous().to(x.dtype)


# ---------------------------------------------------------------------------------------------- frozen BatchNorm (+ add) (+ ReLU)
def bn_chunks(N, C, HW):
    """(chunks per plane, elements per chunk, P) of csrc/bn_act.hip: enough workgroups to fill the device, >= 1024 elements each,
    `per` rounded up to 4 -- chunks * per may overshoot HW, trailing chunks are then empty"""
    planes = N * C
    want = (4096 + planes - 1) // planes
    chunks = max(1, min(want, (HW + 1023) // 1024))
    per = ((HW + chunks - 1) // chunks + 3) // 4 * 4
    return chunks, per, N * chunks


def bn_affine(gamma, beta, mean, var, eps):
    """s, t, invstd in float64 from the fp32 parameters (eps as the fp32 value the kernel receives), and their fp32 error bounds:
    invstd = 1 / sqrt(var + eps) has 3 roundings, s = gamma invstd one more (+ 1 for second-order terms: 5 U |s|);
    t = beta - mean s: the error of s times |mean|, the product and the difference (2 U (|beta| + |mean s|): fused or not)"""
    mean, var = f64(mean), f64(var)
    g = np.ones_like(mean) if gamma is None else f64(gamma)
    b = np.zeros_like(mean) if beta is None else f64(beta)
    invstd = 1.0 / np.sqrt(var + float(f32(eps)))
    s = g * invstd
    t = b - mean * s
    es = 5 * U * np.abs(s)
    et = np.abs(mean) * es + 2 * U * (np.abs(b) + np.abs(mean * s))
    return dict(s=s, t=t, invstd=invstd, es=es, et=et, mean=mean)


def bn_act_forward(x, gamma, beta, mean, var, eps, res, relu):
    """x, res [N, C, HW].  Returns (y, pre-activation, bound) in float64; the bound admits both evaluations of x s + t + r, with and
    without a fused multiply-add: |x| err_s + err_t, one rounding of the product, one of each sum"""
    a = bn_affine(gamma, beta, mean, var, eps)
    x = f64(x)
    s, t = a['s'][None, :, None], a['t'][None, :, None]
    pre = x * s + t
    bound = np.abs(x) * a['es'][None, :, None] + a['et'][None, :, None] + 2 * U * (np.abs(x * s) + np.abs(t))
    if res is not None:
        r = f64(res)
        bound = bound + U * (np.abs(x * s) + np.abs(t) + np.abs(r))
        pre = pre + r
    return (np.maximum(pre, 0.0) if relu else pre), pre, bound


def bn_act_forward_f32(x, gamma, beta, mean, var, eps, res, relu, fused):
    """the kernel's expression in float32, the product either rounded on its own or fused into the sum (evaluated in float64 and
    rounded once: exact for a product of two floats)"""
    C = len(mean)
    g = np.ones(C, f32) if gamma is None else np.asarray(gamma, f32)
    b = np.zeros(C, f32) if beta is None else np.asarray(beta, f32)
    m = np.asarray(mean, f32)
    invstd = f32(1) / np.sqrt(np.asarray(var, f32) + f32(eps))
    s = (g * invstd).astype(f32)
    t = (b.astype(np.float64) - m.astype(np.float64) * s).astype(f32) if fused else b - m * s
    s3, t3 = s[None, :, None], t[None, :, None]
    x = np.asarray(x, f32)
    v = (x.astype(np.float64) * s3 + t3).astype(f32) if fused else x * s3 + t3
    if res is not None:
        v = v + np.asarray(res, f32)
    return np.maximum(v, f32(0)) if relu else v


def relu_window(pre, bound):
    """elements whose float64 pre-activation lies within the forward bound of zero: fp32 may put them on either side"""
    return np.abs(pre) <= bound


def bn_act_backward(gy, x, gamma, beta, mean, var, eps, mask):
    """g' = gy * mask (mask None: no ReLU), grad_x = g' s, grad_res = g', grad_beta[c] = sum g', grad_gamma[c] = invstd sum g' (x - mean),
    float64; with the bound of grad_x (the error of s, one product) and the per-(image, channel) absolute sums the summation bounds
    are counted from: A1 = sum |g'|, A2 = invstd sum |g' (x - mean)| [N, C]"""
    a = bn_affine(gamma, beta, mean, var, eps)
    g, x = f64(gy), f64(x)
    if mask is not None:
        g = g * mask
    s = a['s'][None, :, None]
    xm = x - a['mean'][None, :, None]
    return dict(grad_x=g * s, bound_x=np.abs(g) * a['es'][None, :, None] + U * np.abs(g * s), grad_res=g,
                grad_beta=g.sum((0, 2)), grad_gamma=a['invstd'] * (g * xm).sum((0, 2)),
                gp=g, gxm=g * xm * a['invstd'][None, :, None])


def chunk_sums(a, chunks, per):
    """[N, C, HW] -> ([C, N * chunks] sums, the same of |.|): slot n * chunks + k holds elements [k per, (k + 1) per) of plane (n, c)"""
    N, C, HW = a.shape
    pad = np.zeros((N, C, chunks * per))
    pad[:, :, :HW] = a
    pad = pad.reshape(N, C, chunks, per)
    to_slots = lambda v: v.transpose(1, 0, 2).reshape(C, N * chunks)
    return to_slots(pad.sum(3)), to_slots(np.abs(pad).sum(3))


def bn_act_chain(per):
    """the longest chain of fp32 additions in one workgroup's sum of csrc/bn_act.hip bn_act_bwd_kernel: a lane adds 4 elements per
    trip of 1024 (lane-strided), 6 butterfly steps across the wave, 2 for the four waves"""
    return 4 * ((per + 1023) // 1024) + 6 + 2


def bn_fold_chain(per):
    """relu_sum_bwd_kernel: 3 additions per trip ((v0 + v1) + (v2 + v3), then the accumulator), one ragged element, 6 + 2 as above"""
    return 3 * ((per + 1023) // 1024) + 1 + 6 + 2


def bn_relu_maxpool(x, gamma, beta, mean, var, eps):
    """x [N, C, H, W] -> (maxpool3x3/s2/p1(relu(x s + t)), bound) in float64: the maximum is 1-Lipschitz, so the bound of an output
    is the largest forward bound in its window"""
    N, C, H, W = x.shape
    y, _, bound = bn_act_forward(np.asarray(x).reshape(N, C, H * W), gamma, beta, mean, var, eps, None, True)
    pool = lambda v: F.max_pool2d(torch.from_numpy(v.reshape(N, C, H, W)), 3, 2, 1).numpy()
    return pool(y), pool(bound)


def bn_fold_finish(partial, w, G, s, mean, var, eps):
    """kgdet_bn_fold_finish in float64 from its fp32 inputs: grad_beta = sum partial, grad_gamma = invstd (<w, G> - mean grad_beta),
    grad_w = s G; with the bounds: grad_beta (ceil(P / 256) + 8) U sum |partial|; the dot product one rounding per product more,
    chain ceil(CK / 256); the difference d - mean b (2 roundings, fused or not) and sqrt(var + eps), the division (4)"""
    partial, w, G, s, mean, var = (f64(a) for a in (partial, w, G, s, mean, var))
    O, P = partial.shape
    CK = w.shape[1]
    invstd = 1.0 / np.sqrt(var + float(f32(eps)))
    b = partial.sum(1)
    d = (w * G).sum(1)
    eb = ((P + 255) // 256 + 8) * U * np.abs(partial).sum(1)
    ed = ((CK + 255) // 256 + 9) * U * np.abs(w * G).sum(1)
    gg = invstd * (d - mean * b)
    eg = invstd * (ed + np.abs(mean) * eb + 2 * U * (np.abs(d) + np.abs(mean * b))) + 4 * U * np.abs(gg)
    return dict(grad_beta=b, bound_beta=eb, grad_gamma=gg, bound_gamma=eg, grad_w=G * s[:, None])


# ---------------------------------------------------------------------------------------------- shared inputs of the bn_act tests
BN_EPS = 1e-5
# (N, C, HW): the shapes of test_frozen_bn_act_matches_torch, the ragged and tiny planes, one whose chunks overshoot (HW = 350300:
# 342 chunks of 1028 elements, the last one empty), one with many chunks per plane
BN_SHAPES = [(2, 64, 100 * 168), (2, 256, 50 * 84), (2, 37, 25 * 42), (3, 5, 1), (3, 5, 3), (2, 7, 4), (2, 7, 5), (2, 9, 1023),
             (2, 9, 1024), (2, 9, 1025), (1, 12, 350300), (1, 2, 40000)]


def bn_inputs(N, C, HW, seed=0, with_res=True):
    rng = np.random.default_rng(seed + 7 * HW + C)
    x = (2 * rng.standard_normal((N, C, HW)) + 0.5).astype(f32)
    res = rng.standard_normal((N, C, HW)).astype(f32) if with_res else None
    gy = rng.standard_normal((N, C, HW)).astype(f32)
    gamma, beta = rng.normal(1.0, 0.5, C).astype(f32), rng.normal(0.0, 0.5, C).astype(f32)
    mean, var = rng.normal(0.3, 1.0, C).astype(f32), (0.2 + rng.random(C) * 3).astype(f32)
    return dict(x=x, res=res, gy=gy, gamma=gamma, beta=beta, mean=mean, var=var)


def bn_near_zero_inputs(n=4096, x0=1.7):
    """Two channels whose pre-activation x s + t lands at 0 or within an ulp or two of it; mean = 0, so the kernel's t is exactly beta.
    Channel 0: gamma 0.75, var 0.35, beta = -x0 s computed in float64 from the fp32 s and rounded: the product is inexact, a fused
    and an unfused evaluation may differ in the last place and in the sign.  Channel 1: gamma 0.5 and var + eps == 0.25, s == 1
    exactly, beta = -x0: x s + t = x - x0 is exact either way and every fourth element is exactly 0 (where > and >= part).
    x = the n floats around x0; a residual of 0, +-2^-24, +-2^-23 and +-1.  Returns the arrays [1, 2, n] and the fp32 s."""
    gamma, mean = np.array([0.75, 0.5], f32), np.zeros(2, f32)
    var = np.array([0.35, 0.25 - BN_EPS], f32)
    s = (gamma * (f32(1) / np.sqrt(var + f32(BN_EPS)))).astype(f32)
    beta = (-(np.float64(f32(x0)) * s.astype(np.float64))).astype(f32)
    x = np.full(n, x0, f32)
    for k in range(1, n // 2):
        x[n // 2 + k] = np.nextafter(x[n // 2 + k - 1], f32(10))
        x[n // 2 - k] = np.nextafter(x[n // 2 - k + 1], f32(-10))
    x[0] = np.nextafter(x[1], f32(-10))
    x = np.stack([x, x])
    x[1, ::4] = f32(x0)
    rng = np.random.default_rng(5)
    res = rng.choice(np.array([0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -23, -2.0 ** -23, 1.0, -1.0], f32), (2, n)).astype(f32)
    gy = (rng.standard_normal((2, n)) + 3).astype(f32)
    gy[gy == 0] = 1.0                                              # never 0
    return dict(x=x[None], res=res[None], gy=gy[None], gamma=gamma, beta=beta, mean=mean, var=var), s


def fold_case(seed=0, N=2, Cin=6, O=5, H=9, W=7, k=3):
    """a small real convolution in float64: y = conv(x, w), z = relu(y s + t), the definition grad_gamma = invstd sum g' (y - mean),
    and the inputs of kgdet_bn_fold_finish (the chunk sums of g' and the raw weight gradient G, rounded to fp32)"""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((N, Cin, H, W)))
    w = torch.from_numpy(rng.standard_normal((O, Cin, k, k)).astype(f32)).double().requires_grad_(True)
    gamma, beta = rng.normal(1.0, 0.5, O).astype(f32), rng.normal(0, 0.5, O).astype(f32)
    mean, var = rng.normal(0.3, 1.0, O).astype(f32), (0.2 + rng.random(O) * 3).astype(f32)
    a = bn_affine(gamma, beta, mean, var, BN_EPS)
    y = F.conv2d(x, w, padding=k // 2)
    z = torch.relu(y * torch.from_numpy(a['s'])[None, :, None, None] + torch.from_numpy(a['t'])[None, :, None, None])
    gz = torch.from_numpy(rng.standard_normal(tuple(z.shape)))
    gp = gz * (z > 0)
    (y * gp).sum().backward()                                      # G = the weight gradient of conv(x, .) against g'
    want_gamma = a['invstd'] * (gp * (y.detach() - torch.from_numpy(a['mean'])[None, :, None, None])).sum((0, 2, 3)).numpy()
    chunks, per, P = bn_chunks(N, O, H * W)
    partial, _ = chunk_sums(gp.numpy().reshape(N, O, H * W), chunks, per)
    return dict(partial=partial.astype(f32), w=w.detach().numpy().reshape(O, -1).astype(f32), G=w.grad.numpy().reshape(O, -1).astype(f32),
                s=a['s'].astype(f32), mean=mean, var=var, want_gamma=want_gamma, want_beta=gp.sum((0, 2, 3)).numpy(),
                gp_abs=gp.abs().sum((0, 2, 3)).numpy())


def fold_input_slack(c):
    """what rounding G and the partial sums to fp32 (inputs of the kernel) moves the float64 results by"""
    invstd = 1.0 / np.sqrt(c['var'].astype(np.float64) + float(f32(BN_EPS)))
    eb = U * np.abs(c['partial']).astype(np.float64).sum(1)
    ed = U * np.abs(c['w'].astype(np.float64) * c['G']).sum(1)
    return dict(beta=eb, gamma=invstd * (ed + np.abs(c['mean']) * eb))
