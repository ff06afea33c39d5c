"""Pins the float64 references of tests/step_refs.py (no GPU): each against torch's own CPU operators in float64, the float32
restatements against the float64 ones, and the rounding bounds of tests/test_gpu_step_kernels.py against the restatements."""
import math

import numpy as np
import pytest
import torch

from tests import step_refs as R
from tests import torch_ref


@pytest.mark.parametrize('max_norm', [35.0, 0.05])                  # clip inactive / active
@pytest.mark.parametrize('betas', [(0.9, 0.999), (0.3, 0.9)])
@pytest.mark.parametrize('wd', [0.0, 1e-4])
def test_clip_adam_step_equals_torch_clip_and_adam_in_float64(wd, betas, max_norm):
    rng = np.random.default_rng(3)
    shapes = [(7,), (5, 3), (1,), (33, 2)]
    params = [torch.nn.Parameter(torch.from_numpy(rng.normal(size=s))) for s in shapes]
    opt = torch.optim.Adam(params, lr=1e-2, betas=betas, eps=1e-8, weight_decay=wd, foreach=False)
    state = [(p.detach().numpy().copy(), np.zeros(s), np.zeros(s)) for p, s in zip(params, shapes)]
    for t in range(1, 6):
        grads = [rng.normal(size=s) * 0.3 for s in shapes]
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g.copy())
        norm = R.grad_norm(grads)
        total = torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
        assert abs(float(total) - norm) <= 1e-12 * norm
        assert (R.clip_coef(norm, max_norm) < 1.0) == (max_norm < 1.0)
        opt.step()
        for i, (p, g) in enumerate(zip(params, grads)):
            pn, gn, mn, vn = R.clip_adam_step(state[i][0], g, state[i][1], state[i][2], norm, max_norm, 1e-2, betas[0], betas[1],
                                              1e-8, wd, t)
            st = opt.state[p]
            for name, got, want in (('p', pn, p.detach()), ('g', gn, p.grad), ('m', mn, st['exp_avg']), ('v', vn, st['exp_avg_sq'])):
                want = want.numpy()
                assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (name, t)
            state[i] = (pn, mn, vn)


def test_clip_adam_non_finite_norm_follows_torch():
    """clip_grad_norm_ multiplies every gradient by the clamped coefficient: a NaN norm turns them all into NaN, an infinite
    one into zeros (and the infinite element itself into NaN)"""
    for bad in (float('nan'), float('inf')):
        params = [torch.nn.Parameter(torch.arange(4, dtype=torch.float64) + 1), torch.nn.Parameter(torch.ones(3, dtype=torch.float64))]
        opt = torch.optim.Adam(params, lr=1e-2, foreach=False)
        grads = [np.array([0.5, bad, -1.0, 2.0]), np.array([1.0, 2.0, 3.0])]
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g.copy())
        before = [p.detach().numpy().copy() for p in params]
        with np.errstate(all='ignore'):
            norm = R.grad_norm(grads)
        torch.nn.utils.clip_grad_norm_(params, 35.0, foreach=False)
        opt.step()
        for p, g, b in zip(params, grads, before):
            z = np.zeros_like(b)
            pn, gn, mn, vn = R.clip_adam_step(b, g, z, z, norm, 35.0, 1e-2, 0.9, 0.999, 1e-8, 0.0, 1)
            np.testing.assert_allclose(pn, p.detach().numpy(), rtol=1e-12, equal_nan=True)
            np.testing.assert_allclose(gn, p.grad.numpy(), rtol=1e-12, equal_nan=True)
        assert not np.isfinite(params[0].detach().numpy()[1])
        assert np.isnan(params[1].detach().numpy()).all() == math.isnan(bad)


@pytest.mark.parametrize('wd', [0.0, 1e-4])
@pytest.mark.parametrize('beta1', [0.9, 0.3])
@pytest.mark.parametrize('max_norm', [35.0, 0.05, 0.0])
@pytest.mark.parametrize('t', [1, 2, 1000])
def test_float32_adam_restatement_stays_inside_the_rounding_bounds(t, max_norm, beta1, wd):
    """the (k + 1) 2^-24 bounds the kernel is held to, checked on the operation-by-operation float32 restatement of its expression"""
    f = np.float32
    rng = np.random.default_rng(t)
    n = 200000
    p = rng.normal(size=n).astype(f)
    g = (rng.normal(size=n) * 10.0 ** rng.uniform(-6, 3, n)).astype(f)
    m = (rng.normal(size=n) * 10.0 ** rng.uniform(-6, 1, n)).astype(f)
    v = (rng.random(n) * 10.0 ** rng.uniform(-12, 2, n)).astype(f)
    g[:100] = m[:100] = v[:100] = 0
    norm = f(R.grad_norm([g]))
    lr, eps, wdf, beta2 = float(f(1e-3)), float(f(1e-8)), float(f(wd)), 0.999
    ref = R.clip_adam_step(p, g, m, v, norm, max_norm, lr, beta1, beta2, eps, wdf, t)
    bounds = R.clip_adam_bounds(p, g, m, v, norm, max_norm, lr, beta1, beta2, eps, wdf, t)
    got = R.clip_adam_step_f32(p, g, m, v, norm, max_norm, lr, beta1, beta2, eps, wdf, f(1.0 - beta1 ** t), f(math.sqrt(1.0 - beta2 ** t)))
    for name, a, b, bound in zip('pgmv', (got[0], got[1], got[2], got[3]), ref, (bounds[3], bounds[0], bounds[1], bounds[2])):
        ratio = float((np.abs(a.astype(np.float64) - b) / np.maximum(bound, 1e-300)).max())
        print('%s: restatement error %.3f of its bound' % (name, ratio))
        assert ratio <= 1.0, (name, ratio)
    if wd == 0:
        assert (got[0][:100] == p[:100]).all()


@pytest.mark.parametrize('with_weight', [True, False])
@pytest.mark.parametrize('beta,divisor', [(1.0 / 9.0, 128.0), (1.0, 1.0), (0.5, -32.0)])
def test_smooth_l1_reference_equals_the_torch_chain_in_float64(beta, divisor, with_weight):
    from kgdet_amd import losses
    torch.manual_seed(1)
    shape = (210, 588)
    pred = (torch.randn(shape, dtype=torch.float64) * 40 + 300).requires_grad_()
    target = pred.detach() + torch.randn(shape, dtype=torch.float64) * 20 * (abs(divisor) / 128.0)
    target[::3] = pred.detach()[::3]
    weight = (torch.rand(shape) > 0.7).double() * torch.rand(shape, dtype=torch.double) if with_weight else None
    fused = losses.FUSED_SMOOTH_L1
    losses.FUSED_SMOOTH_L1 = False
    try:
        want = losses.SmoothL1Loss(beta=beta, loss_weight=1.0)(pred, target, weight, avg_factor=1.0, divisor=divisor)
    finally:
        losses.FUSED_SMOOTH_L1 = fused
    want.backward(torch.tensor(0.7, dtype=torch.float64))
    w = None if weight is None else weight.numpy()
    got = R.smooth_l1_sum(pred.detach().numpy(), target.numpy(), w, beta, divisor)
    assert abs(got - float(want)) <= 1e-12 * abs(float(want))
    grad = R.smooth_l1_grad(pred.detach().numpy(), target.numpy(), w, 0.7, beta, divisor)
    assert np.abs(grad - pred.grad.numpy()).max() <= 1e-12 * np.abs(grad).max()
    assert ((grad == 0) == (pred.grad.numpy() == 0)).all()


def test_smooth_l1_dense_inputs_leave_few_elements_at_the_branch_and_the_restatement_inside_the_bar():
    """the share of weighted elements that may sit on either branch stays under the 0.1 % cap of the GPU test (expected ~1e-4:
    the difference has a sigma of 20 / 128, the window a width of ~1e-5); the float32 restatement meets the GPU test's
    element bars on the rest"""
    pred, target, weight = R.dense_smooth_l1_inputs()
    beta, d = float(np.float32(1.0 / 9.0)), 128.0
    sel = weight != 0
    assert 12 * 588 <= int(sel.sum()) <= 12 * 588 + 7 and pred.shape == (33600, 588)
    p, t, w = pred[sel], target[sel], weight[sel]
    window = R.smooth_l1_branch_window(p, t, beta, d)
    assert window.sum() <= 1e-3 * sel.sum(), window.sum()
    zero = R.zero_weight_waves(weight)
    assert 0.95 < zero.mean() < 1.0 and not (zero & sel.reshape(-1)).any()
    terms, grad = R.smooth_l1_f32(p, t, w, 0.37, beta, d)
    x, l = R.smooth_l1_terms(p, t, beta, d)
    ref = R.smooth_l1_grad(p, t, w, float(np.float32(0.37)), beta, d)
    bound = 4 * R.U * np.abs(ref) + np.where(np.abs(x) < beta, (np.abs(p) + np.abs(t)) / d * 2.0 ** -23 / beta * np.abs(0.37 * w / d), 0.0)
    ratio = (np.abs(grad - ref) / np.maximum(bound, 1e-300))[~window].max()
    print('gradient: restatement error %.3f of its bound' % ratio)
    assert ratio <= 1.0
    fwd = np.abs(terms.astype(np.float64) - w * l).sum()
    assert fwd <= (w * (np.abs(p) + np.abs(t)) / d).sum() * 2.0 ** -23 + 2 * R.U * (w * l).sum()


@pytest.mark.parametrize('gamma,alpha', [(2.0, 0.25), (1.5, 0.5), (0.0, 1.0), (2.0, 1.0), (0.0, 0.25)])
def test_focal_reference_equals_py_sigmoid_focal_loss_in_float64(gamma, alpha):
    rng = np.random.default_rng(5)
    n, c = 700, 13
    logits = rng.normal(size=(n, c)) * 3
    logits[0], logits[1], logits[2] = 30.0, -30.0, 0.0
    target = rng.integers(0, c + 1, n)
    target[:3] = [1, 0, 5]
    x = torch.from_numpy(logits).requires_grad_()
    want = torch_ref.py_sigmoid_focal_loss(x, torch.from_numpy(target), gamma, alpha)
    dl = rng.normal(size=(n, c))
    want.backward(torch.from_numpy(dl))
    got = R.focal_forward(logits, target, gamma, alpha)
    assert np.abs(got - want.detach().numpy()).max() <= 1e-12 * np.abs(got).max()
    grad = R.focal_backward(logits, target, dl, gamma, alpha)
    assert np.abs(grad - x.grad.numpy()).max() <= 1e-11 * np.abs(grad).max()
    # labels outside 0..C: -1 ignores the row, C + 5 leaves only negatives
    t2 = np.array([-1, c + 5, 0])
    rows = logits[[0, 1, 1]]
    f = R.focal_forward(rows, t2, gamma, alpha)
    assert (f[0] == 0).all() and (f[1] == f[2]).all() and (alpha == 1.0 or (f[1] > 0).all())
    assert (R.focal_backward(rows, t2, dl[:3], gamma, alpha)[0] == 0).all()


@pytest.mark.parametrize('gamma', [0.0, 1.5, 2.0])
@pytest.mark.parametrize('alpha', [0.25, 0.5, 1.0])
def test_focal_float32_restatement_equals_float64_inside_80(gamma, alpha):
    """the float32 restatement of csrc/focal.hip against float64 to 1e-5 of the output scale for |x| <= 80 (the project's bar for
    the kernel itself); beyond, it saturates as the kernel and the reference's CUDA code do: log(max(p, FLT_MIN))"""
    rng = np.random.default_rng(7)
    n, c = 3000, 13
    logits = (rng.normal(size=(n, c)) * 3).astype(np.float32)
    for i, val in enumerate([0, 1e-8, -1e-8, 16.7, -16.7, 30, -30, 80, -80]):
        logits[2 * i:2 * i + 2] = val
    target = rng.integers(-1, c + 6, n)
    target[:18] = [1, 0] * 9
    dl = rng.normal(size=(n, c)).astype(np.float32)
    for got, want in ((R.focal_forward_f32(logits, target, gamma, alpha), R.focal_forward(logits, target, gamma, alpha)),
                      (R.focal_backward_f32(logits, target, dl, gamma, alpha), R.focal_backward(logits, target, dl, gamma, alpha))):
        assert got.dtype == np.float32 and np.isfinite(got).all()
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    sat = R.focal_forward_f32(np.full((1, c), -104, np.float32), np.array([1]), gamma, alpha)
    assert abs(float(sat[0, 0]) - alpha * -math.log(float(R.FLT_MIN))) < 1e-4


def test_group_norm_reference_statistics_and_per_image_rows():
    import torch.nn.functional as F
    torch.manual_seed(0)
    N, C, G, HW = 3, 12, 4, 10
    x, gy = torch.randn(N, C, HW, dtype=torch.float64) * 3 + 1, torch.randn(N, C, HW, dtype=torch.float64)
    gamma, beta = torch.randn(C, dtype=torch.float64).requires_grad_(), torch.randn(C, dtype=torch.float64).requires_grad_()
    xr = x.clone().requires_grad_()
    y = F.relu(F.group_norm(xr, G, gamma, beta, 1e-5))
    y.backward(gy)
    out = R.group_norm(x.numpy(), gamma.detach().numpy(), beta.detach().numpy(), G, 1e-5, relu_mask=(y > 0).numpy(), grad_y=gy.numpy())
    for got, want in ((out['y'], y), (out['grad_x'], xr.grad), (out['dgamma'].sum(0), gamma.grad), (out['dbeta'].sum(0), beta.grad)):
        assert np.abs(got - want.detach().numpy()).max() <= 1e-12 * np.abs(got).max()
    xg = x.reshape(N * G, -1).numpy()
    np.testing.assert_allclose(out['mean'], xg.mean(1), rtol=1e-13)
    np.testing.assert_allclose(out['rstd'], 1 / np.sqrt(xg.var(1) + 1e-5), rtol=1e-13)
