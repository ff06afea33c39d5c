"""Pins tests/pointwise_refs.py (no GPU): every float64 reference against torch's own CPU operators and autograd in float64, every
float32 / bf16 restatement against its own bound on the inputs tests/test_gpu_pointwise_kernels.py uses, and the 0.1 % cap on
the elements a ReLU comparison may leave out."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pointwise_refs as R

U = R.U
f32 = np.float32
CAP = 1e-3


def _close(a, b, rel=1e-12):
    a, b = R.f64(a), R.f64(b)
    return np.abs(a - b).max() <= rel * max(np.abs(b).max(), 1e-300)


# ============================================================================================ moment box
@pytest.mark.parametrize('regime', R.MOMENT_REGIMES)
@pytest.mark.parametrize('y_first', [0, 1])
@pytest.mark.parametrize('n', [2, 9, 17])
def test_moment_reference_equals_the_torch_chain_in_float64(n, y_first, regime):
    """mean, torch.std (unbiased), exp, cat and autograd, the location whose points coincide included"""
    px, py, transfer, gb = R.moment_inputs(2, n, 65, regime)
    ref = R.moment_f64(px, py, transfer, gb)
    pts = torch.from_numpy(R.moment_pack(px, py, y_first)).double().requires_grad_(True)
    t = torch.from_numpy(transfer).double().requires_grad_(True)
    p = pts.view(2, n, 2, 65)
    yy, xx = (p[:, :, 0], p[:, :, 1]) if y_first else (p[:, :, 1], p[:, :, 0])
    hw, hh = xx.std(1, keepdim=True) * torch.exp(t[0]), yy.std(1, keepdim=True) * torch.exp(t[1])
    mx, my = xx.mean(1, keepdim=True), yy.mean(1, keepdim=True)
    bbox = torch.cat([mx - hw, my - hh, mx + hw, my + hh], 1)
    bbox.backward(torch.from_numpy(gb).double())
    assert _close(ref['bbox'], bbox)
    gpx, gpy = R.moment_unpack(pts.grad.numpy(), y_first)
    # the location whose points coincide: torch.std's own backward fills the 0 / 0 of the deviation term with 0 -- the kernel's
    # choice -- while the same std written as sqrt(var) propagates 0 * inf = NaN (checked below)
    assert np.isfinite(gpx).all() and _close(gpx[0, :, 0], np.full(n, (gb[0, 0, 0].astype(np.float64) + gb[0, 2, 0]) / n))
    assert _close(ref['gpx'], gpx, 1e-9) and _close(ref['gpy'], gpy, 1e-9)
    q = torch.full((n,), 2.0, dtype=torch.float64, requires_grad=True)
    q.var().sqrt().backward()
    assert torch.isnan(q.grad).all()
    assert _close(ref['gt'], t.grad, 1e-9)          # (the std == 0 location adds exactly 0; 1e-9: float64's own cancellation at offset 4096, spread 1e-2)


@pytest.mark.parametrize('regime', R.MOMENT_REGIMES)
@pytest.mark.parametrize('n', R.MOMENT_N)
def test_moment_restatement_at_coinciding_points_and_its_measured_bars(n, regime):
    """The float32 three-pass algorithm at n equal points: the std is exactly 0 (v - mean is exact, n equal residuals sum and
    divide back exactly), the box collapses to the mean, the point gradient is the mean term alone.  Prints the measured bar of
    every output (tests/test_gpu_pointwise_kernels.py holds the kernels to it); the restatement is inside a quarter of it by
    construction, and the bars stay far below what the mutated algorithms do in the offset regime (README)."""
    px, py, transfer, gb = R.moment_inputs(1, n, 64, regime)
    r = R.moment_f32(px, py, transfer, gb)
    assert r['bbox'][0, 0, 0] == r['bbox'][0, 2, 0] and r['bbox'][0, 1, 0] == r['bbox'][0, 3, 0]
    assert abs(float(r['bbox'][0, 0, 0]) - float(f32(R.MOMENT_EQUAL[regime]))) <= n * U * R.MOMENT_EQUAL[regime]
    assert (r['gpx'][0, :, 0] == (gb[0, 0, 0] + gb[0, 2, 0]) / f32(n)).all()
    assert (r['gpy'][0, :, 0] == (gb[0, 1, 0] + gb[0, 3, 0]) / f32(n)).all()
    bar = R.moment_bar(n, regime)
    print('moment n=%d %s: bars in U * scale: %s' % (n, regime, {k: round(v, 1) for k, v in bar.items()}))
    for B, HW in R.MOMENT_SHAPES[:5]:
        e = R.moment_errors(*R.moment_inputs(B, n, HW, regime))
        assert all(e[k] <= bar[k] / 4 for k in e)
    # counted ceilings the measured bars must stay under: bbox and grad_pts (n + 8) roundings of their scale; the transfer
    # gradient a serial sum over at most 33600 locations
    assert bar['bbox'] <= 4 * (n + 8) and bar['gpx'] <= 4 * (n + 8) and bar['gpy'] <= 4 * (n + 8)
    assert bar['gt'] <= 4 * (33600 + n + 8)


# ============================================================================================ glue
@pytest.mark.parametrize('gm', [0.1, 1.0, 0.0])
def test_reppts_offsets_restatement_equals_the_torch_chain(gm):
    rng = np.random.default_rng(0)
    v = (rng.standard_normal((2, 170, 33)) * 4).astype(f32)
    ks = (3, 5, 7)
    outs = R.reppts_offsets_f32(v, ks, gm)
    t = torch.from_numpy(v).requires_grad_(True)
    first = 0
    total = 0
    gs = [rng.standard_normal((2, 2 * k * k, 33)).astype(f32) for k in ks]
    for k, o, g in zip(ks, outs, gs):
        part = t[:, first:first + 2 * k * k]
        part = gm * part + (1 - gm) * part.detach()
        pad = (k - 1) // 2
        yy, xx = torch.meshgrid(torch.arange(-pad, pad + 1.0), torch.arange(-pad, pad + 1.0), indexing='ij')
        base = torch.stack([yy.reshape(-1), xx.reshape(-1)], 1).reshape(1, -1, 1)
        want = part - base
        assert np.array_equal(want.detach().numpy().view(np.int32), o.view(np.int32))
        total = total + (want * torch.from_numpy(g)).sum()
        first += 2 * k * k
    total.backward()
    got = R.reppts_offsets_grad_f32(gs, ks, gm, 2, 170, 33)
    assert np.array_equal(got, t.grad.numpy())          # (values: at gm == 0 autograd's accumulation turns -0 into +0)
    assert (got[:, 166:] == 0).all()
    assert (R.reppts_offsets_grad_f32([gs[0], None, gs[2]], ks, gm, 2, 170, 33)[:, 18:68] == 0).all()


@pytest.mark.parametrize('H,W', [(50, 84), (51, 84), (7, 9), (1, 1), (2, 4)])
def test_subsample2_reference_is_slicing_and_its_autograd(H, W):
    rng = np.random.default_rng(H)
    x = torch.from_numpy(rng.standard_normal((3, H, W))).requires_grad_(True)
    y = x[:, ::2, ::2]
    assert np.array_equal(R.subsample2(x.detach().numpy()), y.detach().numpy())
    gy = rng.standard_normal(tuple(y.shape))
    other = rng.standard_normal((3, H, W))
    (y * torch.from_numpy(gy)).sum().backward()
    assert np.array_equal(R.subsample2_grad(gy, H, W), x.grad.numpy())
    assert np.array_equal(R.subsample2_grad(gy, H, W, other), x.grad.numpy() + other)


@pytest.mark.parametrize('y_first', [0, 1])
def test_pts_from_offsets_reference_is_permute_flip_scale_add(y_first):
    rng = np.random.default_rng(1)
    B, C, HW, stride = 2, 18, 33, 16.0
    pred = torch.from_numpy(rng.standard_normal((B, C, HW))).requires_grad_(True)
    centres = rng.uniform(0, 900, (B, HW, 2))
    p = pred.permute(0, 2, 1).reshape(B, HW, C // 2, 2)
    if y_first:
        p = p.flip(-1)
    pts = (p * stride + torch.from_numpy(centres)[:, :, None, :]).reshape(B, HW, C)
    g = rng.standard_normal((B, HW, C))
    (pts * torch.from_numpy(g)).sum().backward()
    got = R.pts_from_offsets_f32(pred.detach().numpy(), centres, stride, y_first)
    sc = np.abs(pred.detach().numpy()).max() * stride + 900
    assert np.abs(got - pts.detach().numpy()).max() <= 4 * U * sc          # float32 inputs and two roundings
    gg = R.pts_from_offsets_grad_f32(g, stride, y_first)
    assert np.abs(gg - pred.grad.numpy()).max() <= 2 * U * np.abs(g).max() * stride
    # in float32 the restatement IS the torch chain
    p32 = torch.from_numpy(pred.detach().numpy().astype(f32))
    q = p32.permute(0, 2, 1).reshape(B, HW, C // 2, 2)
    if y_first:
        q = q.flip(-1)
    want = (q * stride + torch.from_numpy(centres.astype(f32))[:, :, None, :]).reshape(B, HW, C)
    assert np.array_equal(got.view(np.int32), want.numpy().view(np.int32))


# ============================================================================================ inference epilogues
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('channels_last', [False, True])
def test_bias_act_restatement_is_inside_its_roundings_of_float64(channels_last, dtype):
    """three fp32 roundings (two sums; the clamp is exact) of |x| + |b| + |r|, and for bf16 one rounding to 8 bits (half an ulp: at most 2^-8 of the value)"""
    rng = np.random.default_rng(2)
    shape = (2, 35, 8) if channels_last else (2, 8, 35)
    x = torch.from_numpy(rng.standard_normal(shape).astype(f32) * 3).to(dtype)
    r = torch.from_numpy(rng.standard_normal(shape).astype(f32)).to(dtype)
    b = rng.standard_normal(8).astype(f32)
    for res in (None, r):
        for relu in (0, 1):
            for bias in (None, b):
                got = R.bias_act_restated(x, bias, res, relu, channels_last).double()
                want = R.bias_act_f64(x, bias, res, relu, channels_last)
                mag = x.double().abs() + (0 if res is None else res.double().abs()) + (0 if bias is None else np.abs(b).max())
                bound = 3 * U * mag + (2.0 ** -8 * want.abs() if dtype == torch.bfloat16 else 0)
                assert bool(((got - want).abs() <= bound).all())


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('H,W', [(1, 1), (2, 2), (7, 9)])
def test_bias_relu_maxpool_restatement_is_max_pool2d(H, W, dtype):
    rng = np.random.default_rng(H)
    x = torch.from_numpy(rng.standard_normal((2, H, W, 8)).astype(f32)).to(dtype)
    b = rng.standard_normal(8).astype(f32)
    got = R.bias_relu_maxpool_restated(x, b).double()
    want = F.max_pool2d(torch.relu(x.double() + torch.from_numpy(b).double()).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    bound = 2 * U * (x.double().abs().max() + np.abs(b).max()) + (2.0 ** -8 * want.abs() if dtype == torch.bfloat16 else 0)
    assert got.shape == want.shape and bool(((got - want).abs() <= bound).all())
    assert (R.bias_relu_maxpool_restated(-x.abs(), -np.abs(b)) == 0).all()


# ============================================================================================ frozen BatchNorm
def _torch_bn(d, relu, with_res):
    x = torch.from_numpy(d['x']).double().requires_grad_(True)
    res = torch.from_numpy(d['res']).double().requires_grad_(True) if with_res else None
    gamma, beta = (torch.from_numpy(d[k]).double().requires_grad_(True) for k in ('gamma', 'beta'))
    y = F.batch_norm(x, torch.from_numpy(d['mean']).double(), torch.from_numpy(d['var']).double(), gamma, beta, False, 0.0,
                     float(f32(R.BN_EPS)))
    if with_res:
        y = y + res
    if relu:
        y = torch.relu(y)
    y.backward(torch.from_numpy(d['gy']).double())
    return y, x.grad, (res.grad if with_res else None), gamma.grad, beta.grad


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('with_res', [False, True])
def test_bn_act_reference_equals_batch_norm_add_relu_and_autograd(with_res, relu):
    d = R.bn_inputs(2, 7, 45)
    res = d['res'] if with_res else None
    y, pre, _ = R.bn_act_forward(d['x'], d['gamma'], d['beta'], d['mean'], d['var'], R.BN_EPS, res, relu)
    ty, gx, gr, gg, gbeta = _torch_bn(d, relu, with_res)
    assert _close(y, ty, 1e-13)
    b = R.bn_act_backward(d['gy'], d['x'], d['gamma'], d['beta'], d['mean'], d['var'], R.BN_EPS, (pre > 0) if relu else None)
    assert _close(b['grad_x'], gx) and _close(b['grad_beta'], gbeta) and _close(b['grad_gamma'], gg, 1e-11)
    if with_res:
        assert _close(b['grad_res'], gr)


@pytest.mark.parametrize('shape', R.BN_SHAPES)
def test_bn_act_restatements_inside_the_bound_and_few_elements_at_the_relu(shape):
    """both float32 evaluations of x s + t (+ r), fused and not, on the GPU test's inputs; the elements within the bound of zero
    -- the only ones a ReLU comparison may leave out -- stay under 0.1 % of every tensor"""
    N, C, HW = shape
    d = R.bn_inputs(N, C, HW)
    for res in (None, d['res']):
        y, pre, bound = R.bn_act_forward(d['x'], d['gamma'], d['beta'], d['mean'], d['var'], R.BN_EPS, res, False)
        assert R.relu_window(pre, bound).sum() <= CAP * pre.size
        worst = 0.0
        for fused in (False, True):
            got = R.bn_act_forward_f32(d['x'], d['gamma'], d['beta'], d['mean'], d['var'], R.BN_EPS, res, False, fused)
            worst = max(worst, float((np.abs(got - y) / bound).max()))
        print('bn_act %s res %d: restatements at %.3f of the bound' % (shape, res is not None, worst))
        assert worst <= 1.0


def _tree_sum_f32(v, per):
    """one workgroup's sum as bn_act_bwd_kernel forms it: lane t adds elements 4 t .. 4 t + 3 of every trip of 1024 in order,
    a xor butterfly over the 64 lanes of each wave, the four waves pairwise"""
    pad = np.zeros((per + 1023) // 1024 * 1024, f32)
    pad[:v.size] = v
    lanes = np.zeros(256, f32)
    for trip in pad.reshape(-1, 256, 4):
        for k in range(4):
            lanes = lanes + trip[:, k]
    w = lanes.reshape(4, 64)
    for d in (32, 16, 8, 4, 2, 1):
        w = w + w[:, np.arange(64) ^ d]
    return (w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])


@pytest.mark.parametrize('shape', [(1, 12, 350300), (1, 2, 40000), (2, 9, 1025)])
def test_bn_act_sum_tree_inside_its_counted_bound(shape):
    N, C, HW = shape
    d = R.bn_inputs(N, C, HW)
    chunks, per, P = R.bn_chunks(N, C, HW)
    g = d['gy'].astype(np.float64)
    sums, absum = R.chunk_sums(g, chunks, per)
    L = R.bn_act_chain(per)
    for c in range(C):
        for n in range(N):
            for k in range(chunks):
                got = _tree_sum_f32(d['gy'][n, c, k * per:(k + 1) * per], per)
                assert abs(float(got) - sums[c, n * chunks + k]) <= L * U * absum[c, n * chunks + k]
    assert chunks * per >= HW and (shape != (1, 12, 350300) or (chunks - 1) * per >= HW)          # the last chunk is empty


@pytest.mark.parametrize('H,W', [(1, 1), (7, 9), (13, 8)])
def test_bn_relu_maxpool_reference_is_max_pool2d(H, W):
    d = R.bn_inputs(2, 5, H * W)
    x = d['x'].reshape(2, 5, H, W)
    y, bound = R.bn_relu_maxpool(x, d['gamma'], d['beta'], d['mean'], d['var'], R.BN_EPS)
    t = F.batch_norm(torch.from_numpy(x).double(), torch.from_numpy(d['mean']).double(), torch.from_numpy(d['var']).double(),
                     torch.from_numpy(d['gamma']).double(), torch.from_numpy(d['beta']).double(), False, 0.0, float(f32(R.BN_EPS)))
    want = F.max_pool2d(torch.relu(t), 3, 2, 1)
    assert y.shape == tuple(want.shape) and _close(y, want, 1e-13) and (bound > 0).all()


def test_bn_fold_finish_identity_equals_the_definition():
    """<w[o], G[o]> = sum g' y: grad_gamma needs neither y nor gamma != 0"""
    c = R.fold_case()
    r = R.bn_fold_finish(c['partial'], c['w'], c['G'], c['s'], c['mean'], c['var'], R.BN_EPS)
    # (the fp32 rounding of the inputs G and partial is part of the bound the kernel is held to: fold_input_slack)
    slack = R.fold_input_slack(c)
    assert (np.abs(r['grad_gamma'] - c['want_gamma']) <= slack['gamma']).all()
    assert (np.abs(r['grad_beta'] - c['want_beta']) <= slack['beta']).all()
    assert _close(r['grad_w'], c['G'].astype(np.float64) * c['s'].astype(np.float64)[:, None])


def test_near_zero_inputs_reach_zero_and_both_sides():
    d, s = R.bn_near_zero_inputs()
    pre = d['x'].astype(np.float64)[0] * s.astype(np.float64)[:, None] + d['beta'].astype(np.float64)[:, None]
    ulp = 2.0 ** -23 * np.abs(d['beta']).max()
    assert (np.abs(pre[0]) < ulp).sum() >= 3 and (pre > 0).sum(1).min() > 1000 and (pre < 0).sum(1).min() > 1000
    assert s[1] == 1.0 and (pre[1] == 0).sum() >= 1024
    assert (d['gy'] != 0).all() and (s != 0).all()


@pytest.mark.parametrize('n', [2, 9, 17, 83])
def test_moment_bar_tells_the_algorithm_without_its_residual_pass_apart(n):
    """the offset regime is there for the second pass: without it the serial restatement itself leaves the bar, through the std
    in grad_transfer (by (mean error / spread)^2 / 2, relatively)"""
    e = R.moment_errors(*R.moment_inputs(2, n, 1050, 'offset'), residual=False)
    bar = R.moment_bar(n, 'offset')
    print('n=%d without the residual pass: grad_transfer at %.1f of its bar' % (n, e['gt'] / bar['gt']))
    assert e['gt'] > 2 * bar['gt']
