"""The grouped 3x3 convolutions -- csrc/grouped_conv.hip -- through the C ABI against tests/grouped_conv_refs.py.

Outputs and the workspace are prefilled with NaN and sit between canaries; the input, the weight, the gradient and the bias sit
between NaN-filled guard regions of a larger buffer, so a read outside them that reaches a sum shows up as NaN.

  exact         lattice operands: the bits of the float64 result, all three entry points and the bias + ReLU store;
  accumulation  mixed-scale operands: |got - f64| <= gamma_n * sum |a_i b_i| per element (n = 9 cpg, 9 cpg + 1 with a bias,
                B Ho Wo for the weight gradient); the worst error of every case is printed as a fraction of its bound.
"""
import numpy as np
import pytest
import torch

from tests import grouped_conv_refs as R
from tests.test_gpu_step_kernels import Guarded

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN = float('nan')
OK, E_SHAPE = 0, 1
GUARD = 64


def _L():
    from kgdet_amd import grouped_conv
    return grouped_conv.library()


def _st():
    from kgdet_amd import _lib
    return _lib.raw_stream()


class _In(object):
    """an operand between two NaN-filled guard regions of GUARD floats"""

    def __init__(self, a):
        a = np.ascontiguousarray(a, f32).reshape(-1)
        self.buf = torch.full((2 * GUARD + a.size,), NAN, dtype=torch.float32, device='cuda')
        self.buf[GUARD:GUARD + a.size] = torch.from_numpy(a).cuda()
        self.ptr = self.buf.data_ptr() + 4 * GUARD


def _out(n):
    g = Guarded(max(int(n), 1))
    g.view().fill_(NAN)
    return g


def _p(g):
    return g.buf.data_ptr() + 4 * g.lead


def _get(g, shape):
    return g.view().cpu().numpy().reshape(shape)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.int32)


def _same_bits(got, ref64, tag):
    ref32 = np.asarray(ref64, np.float64).astype(f32)
    assert (ref32.astype(np.float64) == ref64).all(), tag + ': the reference is no float32 number'
    bad = (_bits(got) != _bits(ref32)) & ~((got == 0) & (ref32 == 0))      # (a zero of either sign is a zero)
    assert not bad.any(), '%s: %d of %d elements differ, first at %s: got %r, want %r' % (
        tag, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0])], ref32[tuple(np.argwhere(bad)[0])])


class _Run(object):
    """the three entry points on one case's operands"""

    def __init__(self, c, op):
        self.c, self.C = c, c.groups * c.cpg
        self.Ho, self.Wo = R.out_size(c.H, c.stride), R.out_size(c.W, c.stride)
        self.x, self.w, self.gy, self.bias = _In(op.x), _In(op.w), _In(op.gy), _In(op.bias)
        self.y_shape, self.x_shape, self.w_shape = (c.B, self.C, self.Ho, self.Wo), (c.B, self.C, c.H, c.W), (self.C, c.cpg, 3, 3)

    def forward(self, bias=False, relu=False):
        c, y = self.c, _out(np.prod(self.y_shape))
        rc = _L().kgdet_gconv3x3_forward(self.x.ptr, self.w.ptr, self.bias.ptr if bias else None, _p(y), c.B, self.C, c.cpg, c.H,
                                         c.W, c.stride, 1 if relu else 0, _st())
        assert rc == OK and y.intact()
        return _get(y, self.y_shape)

    def grad_input(self):
        c, gx = self.c, _out(np.prod(self.x_shape))
        rc = _L().kgdet_gconv3x3_grad_input(self.gy.ptr, self.w.ptr, _p(gx), c.B, self.C, c.cpg, c.H, c.W, c.stride, _st())
        assert rc == OK and gx.intact()
        return _get(gx, self.x_shape)

    def grad_weight(self):
        c, gw = self.c, _out(np.prod(self.w_shape))
        n = _L().kgdet_gconv3x3_workspace_bytes(c.B, self.C, c.cpg, c.H, c.W, c.stride)
        assert n > 0 and n % 4 == 0
        ws = _out(n // 4)
        rc = _L().kgdet_gconv3x3_grad_weight(self.gy.ptr, self.x.ptr, _p(gw), c.B, self.C, c.cpg, c.H, c.W, c.stride, _p(ws), n,
                                             _st())
        assert rc == OK and gw.intact() and ws.intact()
        return _get(gw, self.w_shape)


@pytest.mark.parametrize('name', R.NAMES)
def test_exact_tier_returns_the_bits_of_the_float64_result(name):
    c, op = R.BY_NAME[name], R.lattice(name)
    (fwd, gi, gw), _ = R.results(name, 'lattice')
    run = _Run(c, op)
    _same_bits(run.forward(), fwd, name + ' forward')
    _same_bits(run.grad_input(), gi, name + ' grad_input')
    _same_bits(run.grad_weight(), gw, name + ' grad_weight')
    biased = fwd + op.bias.astype(np.float64)[None, :, None, None]
    _same_bits(run.forward(bias=True), biased, name + ' forward + bias')
    _same_bits(run.forward(bias=True, relu=True), np.maximum(biased, 0.0), name + ' forward + bias + relu')
    _same_bits(run.forward(relu=True), np.maximum(fwd, 0.0), name + ' forward + relu')


def _fraction(got, ref, bound, tag):
    assert np.isfinite(got).all(), tag + ': non-finite results (a read outside an operand?)'
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(all='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    r = float(r.max()) if r.size else 0.0
    print('%s: worst error %.3f of its bound' % (tag, r))
    return r


@pytest.mark.parametrize('name', R.NAMES)
def test_accumulation_tier_stays_inside_the_summation_bound(name):
    c, op = R.BY_NAME[name], R.mixed(name)
    (fwd, gi, gw), (mf, mi, mw) = R.results(name, 'mixed')
    n_f, n_i, n_w = R.summands(c)
    run = _Run(c, op)
    worst = [_fraction(run.forward(), fwd, R.gamma(n_f) * mf, name + ' forward'),
             _fraction(run.grad_input(), gi, R.gamma(n_i) * mi, name + ' grad_input'),
             _fraction(run.grad_weight(), gw, R.gamma(n_w) * mw, name + ' grad_weight')]
    # bias + ReLU: max(0, .) of the biased sum under the bound of one more summand; exact zeros where the float64
    # pre-activation lies below minus the bound
    b64 = op.bias.astype(np.float64)[None, :, None, None]
    pre, bound = fwd + b64, R.gamma(n_f + 1) * (mf + np.abs(b64))
    got = run.forward(bias=True, relu=True)
    worst.append(_fraction(got, np.maximum(pre, 0.0), bound, name + ' forward + bias + relu'))
    assert (got[pre < -bound] == 0).all() and (got >= 0).all()
    worst.append(_fraction(run.forward(bias=True), pre, bound, name + ' forward + bias'))
    assert max(worst) <= 1.0


REPEAT = ['c4_s1_g3_b3_65x129', 'c4_s2_g3_b3_65x129', 'c32_s1_g3_b3_65x129', 'c32_s2_g3_b3_17x33', 'c8_s2_g3_b1_33x65',
          'c16_s1_g3_b3_17x33']


@pytest.mark.parametrize('name', REPEAT)
def test_every_entry_point_repeats_its_bits(name):
    c, op = R.BY_NAME[name], R.mixed(name)
    run = _Run(c, op)
    for fn in (run.forward, run.grad_input, run.grad_weight):
        a, b = fn(), fn()
        assert (_bits(a) == _bits(b)).all(), name + ' ' + fn.__name__
    a = run.grad_weight()
    other = torch.randn(1 << 20, device='cuda')          # an unrelated launch in between
    other.mul_(2.0)
    assert (_bits(a) == _bits(run.grad_weight())).all()


def _refusals():
    """(tag, overrides of a good call's arguments)"""
    return [('cpg 5', dict(cpg=5, C=10)), ('cpg 2', dict(cpg=2, C=8)), ('cpg 64', dict(cpg=64, C=64)),
            ('C not a multiple of cpg', dict(C=6)), ('stride 0', dict(stride=0)), ('stride 3', dict(stride=3)),
            ('B 0', dict(B=0)), ('H 0', dict(H=0)), ('W 0', dict(W=0)),
            ('null a', dict(null='a')), ('null b', dict(null='b')), ('null out', dict(null='out')),
            ('out is a', dict(alias='a')), ('out is b', dict(alias='b')), ('out inside a', dict(alias='a', shift=16))]


@pytest.mark.parametrize('tag,over', _refusals(), ids=[t for t, _ in _refusals()])
def test_refusals_return_shape_error_and_write_nothing(tag, over):
    L = _L()
    a = dict(B=2, C=8, cpg=4, H=5, W=7, stride=1)
    n_map, n_w = 2 * 8 * 5 * 7, 8 * 4 * 9
    a.update({k: v for k, v in over.items() if k in a})
    for entry in ('forward', 'grad_input', 'grad_weight'):
        # operands big enough for the good call; every buffer a Guarded of NaN so that "untouched" can be checked on all
        bufs = {k: _out(max(n_map, n_w) + 32) for k in ('a', 'b', 'out', 'ws', 'bias')}
        ptr = {k: _p(v) for k, v in bufs.items()}
        if over.get('null'):
            ptr[over['null']] = None
        if over.get('alias'):
            ptr['out'] = ptr[over['alias']] + 4 * over.get('shift', 0)
        dims = (a['B'], a['C'], a['cpg'], a['H'], a['W'], a['stride'])
        if entry == 'forward':
            rc = L.kgdet_gconv3x3_forward(ptr['a'], ptr['b'], ptr['bias'], ptr['out'], *dims, 1, _st())
        elif entry == 'grad_input':
            rc = L.kgdet_gconv3x3_grad_input(ptr['a'], ptr['b'], ptr['out'], *dims, _st())
        else:
            rc = L.kgdet_gconv3x3_grad_weight(ptr['a'], ptr['b'], ptr['out'], *dims, ptr['ws'], 4 * (n_w + 32), _st())
        assert rc == E_SHAPE, '%s %s: status %d' % (entry, tag, rc)
        torch.cuda.synchronize()
        for k, g in bufs.items():
            assert g.intact() and bool(torch.isnan(g.view()).all()), '%s %s: %s was written' % (entry, tag, k)


def test_grad_weight_refuses_a_missing_or_short_workspace():
    from kgdet_amd import _lib
    L = _L()
    bufs = {k: _out(1024) for k in ('gy', 'x', 'gw', 'ws')}
    n = L.kgdet_gconv3x3_workspace_bytes(2, 8, 4, 5, 7, 1)
    assert L.kgdet_gconv3x3_workspace_bytes(2, 8, 5, 5, 7, 1) == 0
    rc = L.kgdet_gconv3x3_grad_weight(_p(bufs['gy']), _p(bufs['x']), _p(bufs['gw']), 2, 8, 4, 5, 7, 1, None, n, _st())
    assert rc == E_SHAPE
    rc = L.kgdet_gconv3x3_grad_weight(_p(bufs['gy']), _p(bufs['x']), _p(bufs['gw']), 2, 8, 4, 5, 7, 1, _p(bufs['ws']), n - 4, _st())
    assert rc == _lib.KGDET_E_WORKSPACE
    torch.cuda.synchronize()
    for k, g in bufs.items():
        assert g.intact() and bool(torch.isnan(g.view()).all()), k


def test_op_counts_its_launches_and_matches_the_abi(monkeypatch):
    """grouped_conv.conv3x3 (autograd) and conv3x3_bias_act give what the entry points give, and count their launches"""
    from kgdet_amd import grouped_conv as G
    monkeypatch.setattr(G, 'ENABLED', True)
    name = 'c8_s2_g3_b3_17x33'
    c, op = R.BY_NAME[name], R.mixed(name)
    run = _Run(c, op)
    x = torch.from_numpy(op.x).cuda().requires_grad_(True)
    w = torch.from_numpy(op.w).cuda().requires_grad_(True)
    assert G.applicable(x, w, (c.stride, c.stride), (1, 1), (1, 1), c.groups)
    G.reset_calls()
    y = G.conv3x3(x, w, c.stride)
    y.backward(torch.from_numpy(op.gy).cuda())
    assert G.calls == dict(forward=1, bias_act=0, grad_input=1, grad_weight=1)
    assert (_bits(y.detach().cpu().numpy()) == _bits(run.forward())).all()
    assert (_bits(x.grad.cpu().numpy()) == _bits(run.grad_input())).all()
    assert (_bits(w.grad.cpu().numpy()) == _bits(run.grad_weight())).all()
    with torch.no_grad():
        z = G.conv3x3_bias_act(x, w, torch.from_numpy(op.bias).cuda(), c.stride, relu=True)
    assert G.calls['bias_act'] == 1
    assert (_bits(z.cpu().numpy()) == _bits(run.forward(bias=True, relu=True))).all()
    # outside the envelope, on the GPU
    for bad in (dict(stride=(1, 2)), dict(stride=(3, 3)), dict(padding=(0, 0)), dict(dilation=(2, 2)), dict(groups=1)):
        args = dict(stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=c.groups)
        args.update(bad)
        assert not G.applicable(x, w, **args)
    assert not G.applicable(x.double(), w.double(), (1, 1), (1, 1), (1, 1), c.groups)
    assert not G.applicable(x.detach().permute(0, 1, 3, 2), w, (1, 1), (1, 1), (1, 1), c.groups)
    assert not G.applicable(x, torch.zeros(c.groups * 5, 5, 3, 3, device='cuda'), (1, 1), (1, 1), (1, 1), c.groups)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        assert not G.applicable(x, w, (1, 1), (1, 1), (1, 1), c.groups)
    # a class that stays on torch by default is routed only when forced; the switch takes every class off the route
    x16, w16 = torch.zeros(1, 48, 5, 7, device='cuda'), torch.zeros(48, 16, 3, 3, device='cuda')
    monkeypatch.setattr(G, 'TORCH_CLASSES', frozenset([(16, 1)]))
    monkeypatch.setattr(G, 'FORCE', False)
    assert not G.applicable(x16, w16, (1, 1), (1, 1), (1, 1), 3) and G.applicable(x16, w16, (2, 2), (1, 1), (1, 1), 3)
    monkeypatch.setattr(G, 'FORCE', True)
    assert G.applicable(x16, w16, (1, 1), (1, 1), (1, 1), 3)
    monkeypatch.setattr(G, 'ENABLED', False)
    assert not G.applicable(x16, w16, (1, 1), (1, 1), (1, 1), 3) and not G.applicable(x, w, (2, 2), (1, 1), (1, 1), c.groups)
