"""The float64 reference of the fused clip + SGD step against torch's own CPU operators, its fp32 restatement against the
rounding bounds on the tables the GPU test uploads, and the conditions under which the fused step applies.  No GPU."""
import numpy as np
import pytest
import torch

from tests import sgd_refs as S
from tests.step_refs import clip_coef


@pytest.mark.parametrize('max_norm', [1e3, 0.05])                      # inactive, active
@pytest.mark.parametrize('momentum,wd,dampening,nesterov', [c for c in S.grid() if S.torch_accepts(c[0], c[2], c[3])])
def test_reference_is_torch_clip_and_sgd_in_float64(momentum, wd, dampening, nesterov, max_norm):
    """two consecutive steps of clip_grad_norm_ + torch.optim.SGD(foreach=False) on float64 CPU tensors: the first creates the
    momentum buffers (buf = None in the reference), the second uses them"""
    rng = np.random.default_rng(7)
    shapes = [(5, 3), (17,), (2, 2, 4)]
    params = [torch.nn.Parameter(torch.from_numpy(rng.normal(size=s))) for s in shapes]
    opt = torch.optim.SGD(params, lr=5e-3, momentum=momentum, weight_decay=wd, dampening=dampening, nesterov=nesterov,
                          foreach=False)
    bufs = [None] * len(params)
    for step in range(2):
        grads = [rng.normal(size=s) * 10.0 ** rng.uniform(-3, 1, s) for s in shapes]
        before = [p.detach().numpy().copy() for p in params]
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g.copy())
        norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm=max_norm, norm_type=2))
        assert (clip_coef(norm, max_norm) < 1.0) == (max_norm < 1.0)
        opt.step()
        for i, p in enumerate(params):
            pn, gn, bn = S.clip_sgd_step(before[i], grads[i], bufs[i], norm, max_norm, 5e-3, momentum, dampening, wd, nesterov)
            bufs[i] = bn
            np.testing.assert_allclose(p.detach().numpy(), pn, rtol=1e-12, atol=0)
            np.testing.assert_allclose(p.grad.numpy(), gn, rtol=1e-12, atol=0)
            if momentum != 0:
                np.testing.assert_allclose(opt.state[p]['momentum_buffer'].numpy(), bn, rtol=1e-12, atol=0)
            else:
                assert 'momentum_buffer' not in opt.state[p] or opt.state[p]['momentum_buffer'] is None


@pytest.fixture(scope='module')
def table():
    tb = S.step_table()
    return tb, tb.gather(), tb.grad_norm()


@pytest.mark.parametrize('max_norm', S.MAX_NORMS)
@pytest.mark.parametrize('momentum,wd,dampening,nesterov', S.grid())
def test_fp32_restatement_stays_inside_the_bounds(table, momentum, wd, dampening, nesterov, max_norm):
    """the kernel's expression with one float32 rounding per operation, on the GPU test's table: a correct fp32 kernel passes"""
    tb, (p, g, b), norm = table
    norm = float(np.float32(norm)) if max_norm > 0 else None
    assert max_norm == 0 or (clip_coef(norm, max_norm) < 1.0) == (max_norm < 1.0)
    args = (norm, max_norm, S.LR, momentum, dampening, wd, nesterov)
    ref = S.clip_sgd_step(p, g, b, *args)
    got = S.clip_sgd_step_f32(p, g, b, 0.0 if norm is None else norm, *args[1:])
    bounds = S.clip_sgd_bounds(p, g, b, *args)
    for name, r, x, bound in zip(('grad', 'buffer', 'param'), (ref[1], ref[2], ref[0]), (got[1], got[2], got[0]),
                                 bounds):
        err = np.abs(x.astype(np.float64) - r)
        with np.errstate(all='ignore'):
            ratio = float(np.max(np.where(err == 0, 0.0, err / bound)))
        print('%s: error %.3f of its bound' % (name, ratio))
        assert ratio <= 1.0, name
    if momentum == 0:
        assert (got[2] == b).all()


class _FakeCuda(object):
    """``applicable`` looks at tensors through optim._dense_f32_cuda: with that test standing for 'a CUDA fp32 dense tensor',
    the remaining conditions can be told apart on a machine without a GPU"""

    def __init__(self, monkeypatch):
        from kgdet_amd import optim
        monkeypatch.setattr(optim, '_dense_f32_cuda',
                            lambda t: isinstance(t, torch.Tensor) and t.dtype == torch.float32 and not t.is_sparse and t.is_contiguous())


def _stepped(n_groups=1, momentum=0.9, **kw):
    params = [torch.nn.Parameter(torch.randn(3, 5)), torch.nn.Parameter(torch.randn(7))]
    groups = [dict(params=params)] if n_groups == 1 else [dict(params=[p]) for p in params]
    opt = torch.optim.SGD(groups, lr=5e-3, momentum=momentum, weight_decay=1e-4, **kw)
    for p in params:
        p.grad = torch.randn_like(p)
    opt.step()                                  # creates the momentum buffers
    return opt, params


def test_fused_clip_sgd_applies_only_where_the_issue_says(monkeypatch):
    from kgdet_amd.optim import FusedClipSGD
    clip = dict(max_norm=35, norm_type=2)
    opt, params = _stepped()
    assert not FusedClipSGD.applicable(opt, params, clip)               # CPU parameters
    _FakeCuda(monkeypatch)
    assert FusedClipSGD.applicable(opt, params, clip)                   # ... and nothing else stands in the way
    assert FusedClipSGD.applicable(opt, params, None)
    assert FusedClipSGD.applicable(*_stepped(momentum=0.0), clip)
    assert FusedClipSGD.applicable(*_stepped(nesterov=True), clip)
    assert not FusedClipSGD.applicable(opt, params, dict(max_norm=35, norm_type=1))
    assert not FusedClipSGD.applicable(*_stepped(maximize=True), clip)
    assert not FusedClipSGD.applicable(*_stepped(n_groups=2), clip)
    opt_t, params_t = _stepped()
    opt_t.param_groups[0]['lr'] = torch.tensor(5e-3)
    assert not FusedClipSGD.applicable(opt_t, params_t, clip)
    opt_f, params_f = _stepped()
    opt_f.param_groups[0]['fused'] = True                               # (what SGD(fused=True) leaves in the group)
    assert not FusedClipSGD.applicable(opt_f, params_f, clip)
    params_n = [torch.nn.Parameter(torch.randn(3, 5))]
    opt_n = torch.optim.SGD(params_n, lr=5e-3, momentum=0.9)
    params_n[0].grad = torch.randn(3, 5)
    assert not FusedClipSGD.applicable(opt_n, params_n, clip)           # no momentum buffers yet: the first step is torch's
    assert not FusedClipSGD.applicable(torch.optim.Adam(params_n, lr=1e-3), params_n, clip)
    half = [torch.nn.Parameter(torch.randn(4).double())]
    opt_h = torch.optim.SGD(half, lr=5e-3)
    half[0].grad = torch.randn(4).double()
    assert not FusedClipSGD.applicable(opt_h, half, clip)               # not fp32
