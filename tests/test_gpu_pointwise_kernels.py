"""The small kernels between the convolutions of every step -- csrc/moment.hip, glue.hip, epilogue.hip, bn_act.hip -- through the
C ABI (ctypes, not the Python wrappers: those filter out the argument combinations of interest) against tests/pointwise_refs.py:
bit-equal to the float32 / bf16 restatement where the kernel promises it, inside a bound counted from the kernel's expression
(U = 2^-24 per rounding) otherwise, inside the measured bar (pointwise_refs.moment_bar) for the moment box.  Every output sits
inside a buffer of a canary value that must stay untouched, pre-filled with NaN where the kernel claims to write every element.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import pointwise_refs as R
from tests.test_gpu_step_kernels import CANARY, Guarded, _L, _bit_equal, _ptr, _ratio

pytestmark = pytest.mark.gpu

U = R.U
f32 = np.float32
NAN = float('nan')
c_f, c_i32, c_i64, c_sz = ctypes.c_float, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
E_SHAPE, E_UNSUPPORTED = 1, 4


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _out(n, fill=NAN):
    g = Guarded(n)
    if fill is not None:
        g.view().fill_(fill)
    return g


def _st():
    return _L()[0].current_stream()


def _np_bits_equal(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


# ============================================================================================ moment box
@functools.lru_cache(maxsize=2)
def _moment_ref(B, n, HW, regime):
    inp = R.moment_inputs(B, n, HW, regime)
    return inp, R.moment_f64(*inp)


def _moment_run(pts, transfer, gb, B, n, HW, y_first):
    lib, L = _L()
    bbox = _out(B * 4 * HW)
    lib.check(L.kgdet_moment_bbox_forward(_ptr(pts), _ptr(transfer), c_i32(B), c_i32(n), c_i32(HW), c_i32(y_first), bbox.ptr(), _st()),
              'moment_bbox_forward')
    assert bbox.intact()
    wsb = L.kgdet_moment_bbox_backward_workspace_bytes(c_i32(B), c_i32(HW))
    assert wsb % 4 == 0 and wsb >= (B * HW + 63) // 64 * 8
    outs = []
    for _ in range(2):
        gp, gt, ws = _out(B * 2 * n * HW), _out(2), Guarded(wsb // 4)         # the workspace exactly as large as asked for
        lib.check(L.kgdet_moment_bbox_backward(_ptr(pts), _ptr(transfer), _ptr(gb), c_i32(B), c_i32(n), c_i32(HW), c_i32(y_first),
                                               gp.ptr(), gt.ptr(), ws.ptr(), c_sz(wsb), _st()), 'moment_bbox_backward')
        assert gp.intact() and gt.intact() and ws.intact()
        outs.append((gp.view().clone(), gt.view().clone()))
    assert _bit_equal(outs[0][0], outs[1][0]) and _bit_equal(outs[0][1], outs[1][1])          # no float atomics
    return (bbox.view().cpu().numpy().reshape(B, 4, HW), outs[0][0].cpu().numpy().reshape(B, 2 * n, HW), outs[0][1].cpu().numpy())


def _moment_cases():
    return [(B, HW, n) for n in R.MOMENT_N for B, HW in R.moment_shapes(n)]


@pytest.mark.parametrize('regime', R.MOMENT_REGIMES)
@pytest.mark.parametrize('y_first', [0, 1])
@pytest.mark.parametrize('B,HW,n', _moment_cases())
def test_moment_bbox_against_float64(B, HW, n, y_first, regime):
    """Forward and backward at every n either side of the 16-wave split and every B * HW around a block of 64, zero-mean points
    and points with a common offset of 2048 .. 4096 around a spread of 1e-2 .. 1e-1 -- where the residual pass of the mean decides the
    std: without it grad_transfer is off by (mean error / spread)^2 / 2, thousands of times the bar.  The bar is measured, not
    counted: pointwise_refs.moment_bar, 4 x the serial float32 restatement's own error over the inputs of this n and regime.
    Location 0 holds n equal points: the box collapses to the mean and grad_pts is the mean term alone, finite -- as
    torch.std's backward fills it (sqrt(var) written out would give NaN: 0 * inf); kept because one degenerate location must not
    poison the step's gradients."""
    (px, py, transfer, gb), ref = _moment_ref(B, n, HW, regime)
    pts = _dev(R.moment_pack(px, py, y_first))
    bbox, gp, gt = _moment_run(pts, _dev(transfer), _dev(gb), B, n, HW, y_first)
    assert np.isfinite(bbox).all() and np.isfinite(gp).all() and np.isfinite(gt).all()          # every element written
    gpx, gpy = R.moment_unpack(gp, y_first)
    bar = R.moment_bar(n, regime)
    tag = 'moment B%d HW%d n%d yf%d %s ' % (B, HW, n, y_first, regime)
    worst = {k: _ratio(got, ref[k], bar[k] * U * ref['scale_' + k], tag + k)
             for k, got in (('bbox', bbox), ('gpx', gpx), ('gpy', gpy), ('gt', gt))}
    assert max(worst.values()) <= 1.0, worst
    if B * HW > 1:
        assert bbox[0, 0, 0] == bbox[0, 2, 0] and bbox[0, 1, 0] == bbox[0, 3, 0]
        assert (gpx[0, :, 0] == (gb[0, 0, 0] + gb[0, 2, 0]) / f32(n)).all() and (gpy[0, :, 0] == (gb[0, 1, 0] + gb[0, 3, 0]) / f32(n)).all()


@pytest.mark.parametrize('n', R.MOMENT_N)
def test_moment_bbox_single_location_of_equal_points(n):
    px = np.full((1, n, 1), 4001.7, f32)
    py = np.full((1, n, 1), -37.3, f32)
    gb = np.array([0.5, -1.25, 2.0, 0.75], f32).reshape(1, 4, 1)
    for y_first in (0, 1):
        bbox, gp, gt = _moment_run(_dev(R.moment_pack(px, py, y_first)), _dev(np.array([0.3, -0.2], f32)), _dev(gb), 1, n, 1, y_first)
        assert bbox[0, 0, 0] == bbox[0, 2, 0] and abs(float(bbox[0, 0, 0]) - float(px[0, 0, 0])) <= n * U * 4001.7
        assert bbox[0, 1, 0] == bbox[0, 3, 0] and abs(float(bbox[0, 1, 0]) - float(py[0, 0, 0])) <= n * U * 37.3
        gpx, gpy = R.moment_unpack(gp, y_first)
        assert (gpx == f32(2.5) / f32(n)).all() and (gpy == f32(-0.5) / f32(n)).all()
        assert (gt == 0).all()


def test_moment_bbox_refuses_one_point_and_leaves_an_empty_map_alone():
    lib, L = _L()
    pts, t, gb = torch.zeros(64, device='cuda'), torch.zeros(2, device='cuda'), torch.zeros(64, device='cuda')
    for B, n, HW, want in ((1, 1, 8, E_SHAPE), (0, 9, 8, 0), (2, 9, 0, 0)):
        bbox, gp, gt, ws = Guarded(64), Guarded(64), Guarded(2), Guarded(16)
        assert L.kgdet_moment_bbox_forward(_ptr(pts), _ptr(t), c_i32(B), c_i32(n), c_i32(HW), c_i32(1), bbox.ptr(), _st()) == want
        assert L.kgdet_moment_bbox_backward(_ptr(pts), _ptr(t), _ptr(gb), c_i32(B), c_i32(n), c_i32(HW), c_i32(1), gp.ptr(), gt.ptr(),
                                            ws.ptr(), c_sz(64), _st()) == want
        torch.cuda.synchronize()
        for g in (bbox, gp, gt, ws):
            assert (g.buf == CANARY).all()


# ============================================================================================ glue
KS = (3, 5, 7)


def _ks():
    return (c_i32 * 3)(*KS)


@pytest.mark.parametrize('B,C,HW,gm', [(8, 166, 50 * 84, 0.1), (2, 170, 1050, 1.0), (1, 200, 63, 0.0), (3, 170, 1, 0.1)])
def test_reppts_offsets_forward_bit_exact(B, C, HW, gm):
    """[8, 166, 50, 84] is 5.6 M elements: the launch is capped at 2048 x 256 threads, the stride loop makes eleven trips"""
    lib, L = _L()
    rng = np.random.default_rng(C + HW)
    v = (rng.standard_normal((B, C, HW)) * 4).astype(f32)
    outs = [_out(B * 2 * k * k * HW) for k in KS]
    dv = _dev(v)
    lib.check(L.kgdet_reppts_offsets_forward(_ptr(dv), c_i32(B), c_i32(C), c_i32(HW), _ks(), c_f(gm), outs[0].ptr(), outs[1].ptr(),
                                             outs[2].ptr(), _st()), 'reppts_offsets_forward')
    for o, want in zip(outs, R.reppts_offsets_f32(v, KS, gm)):
        assert o.intact()                     # (channels past the three slices have nowhere to go)
        assert _np_bits_equal(o.view().cpu().numpy().reshape(want.shape), want)


@pytest.mark.parametrize('B,C,HW,gm,nulls', [(8, 166, 50 * 84, 0.1, ())] + [(2, 170, 130, (0.1, 1.0, 0.0)[k % 3], tuple(j for j in range(3) if k >> j & 1))
                                                                          for k in range(8)] + [(1, 200, 63, 1.0, (1,))])
def test_reppts_offsets_backward_bit_exact(B, C, HW, gm, nulls):
    lib, L = _L()
    rng = np.random.default_rng(C + HW + len(nulls))
    gs = [None if j in nulls else rng.standard_normal((B, 2 * k * k, HW)).astype(f32) for j, k in enumerate(KS)]
    dg = [_dev(g) for g in gs]
    out = _out(B * C * HW)
    lib.check(L.kgdet_reppts_offsets_backward(_ptr(dg[0]), _ptr(dg[1]), _ptr(dg[2]), c_i32(B), c_i32(C), c_i32(HW), _ks(), c_f(gm),
                                              out.ptr(), _st()), 'reppts_offsets_backward')
    assert out.intact()
    got = out.view().cpu().numpy().reshape(B, C, HW)
    assert _np_bits_equal(got, R.reppts_offsets_grad_f32(gs, KS, gm, B, C, HW))
    assert (got[:, 166:].view(np.int32) == 0).all()          # exactly +0 beyond the slices


def test_reppts_offsets_refuse_too_few_channels():
    lib, L = _L()
    v, out = torch.zeros(165 * 4, device='cuda'), Guarded(165 * 4)
    assert L.kgdet_reppts_offsets_forward(_ptr(v), c_i32(1), c_i32(165), c_i32(4), _ks(), c_f(0.1), out.ptr(), out.ptr(), out.ptr(),
                                          _st()) == E_SHAPE
    assert L.kgdet_reppts_offsets_backward(_ptr(v), _ptr(v), _ptr(v), c_i32(1), c_i32(165), c_i32(4), _ks(), c_f(0.1), out.ptr(),
                                           _st()) == E_SHAPE
    torch.cuda.synchronize()
    assert (out.buf == CANARY).all()


@pytest.mark.parametrize('planes,H,W', [(7, 50, 84), (7, 51, 84), (5, 7, 9), (3, 1, 1), (3, 2, 4), (1024, 50, 84)])
def test_subsample2_forward_bit_exact(planes, H, W):
    """odd H and odd W included (the ABI accepts both); 1024 planes of 50 x 84 give 1.08 M outputs, beyond 4096 x 256 threads"""
    lib, L = _L()
    x = np.random.default_rng(H * W).standard_normal((planes, H, W)).astype(f32)
    want = R.subsample2(x)
    y, dx = _out(want.size), _dev(x)
    lib.check(L.kgdet_subsample2_forward(_ptr(dx), y.ptr(), c_i64(planes), c_i32(H), c_i32(W), _st()), 'subsample2_forward')
    assert y.intact() and _np_bits_equal(y.view().cpu().numpy().reshape(want.shape), want)


@pytest.mark.parametrize('with_other', [False, True])
@pytest.mark.parametrize('planes,H,W', [(7, 50, 84), (7, 51, 84), (3, 2, 4), (3, 1, 4), (5, 7, 8), (2048, 50, 84)])
def test_subsample2_backward_bit_exact(planes, H, W, with_other):
    """the accumulate argument `other` of the ABI, null and not; 2048 planes of 50 x 84 are 2.15 M float4, beyond 8192 x 256"""
    lib, L = _L()
    rng = np.random.default_rng(H * W + planes)
    gy = rng.standard_normal((planes, (H + 1) // 2, W // 2)).astype(f32)
    other = rng.standard_normal((planes, H, W)).astype(f32) if with_other else None
    gx, dgy, dother = _out(planes * H * W), _dev(gy), _dev(other)
    lib.check(L.kgdet_subsample2_backward(_ptr(dgy), _ptr(dother), gx.ptr(), c_i64(planes), c_i32(H), c_i32(W), _st()),
              'subsample2_backward')
    got = gx.view().cpu().numpy().reshape(planes, H, W)
    assert gx.intact() and _np_bits_equal(got, R.subsample2_grad(gy, H, W, other))


def test_subsample2_backward_refuses_a_width_not_a_multiple_of_4():
    lib, L = _L()
    gy, gx = torch.zeros(64, device='cuda'), Guarded(64)
    assert L.kgdet_subsample2_backward(_ptr(gy), None, gx.ptr(), c_i64(1), c_i32(4), c_i32(6), _st()) == E_SHAPE
    torch.cuda.synchronize()
    assert (gx.buf == CANARY).all()


PTS_C = [2, 18, 62, 64, 66, 130, 588]
PTS_HW = [1, 31, 32, 33, 1050, 16800]


@pytest.mark.parametrize('y_first', [0, 1])
@pytest.mark.parametrize('C,HW', [(C, HW) for C in PTS_C for HW in PTS_HW])
def test_pts_from_offsets_bit_exact(C, HW, y_first):
    lib, L = _L()
    k = PTS_C.index(C) + PTS_HW.index(HW)
    B = 3 if C * HW <= 200000 else (2 if HW <= 1050 else 1)
    stride = float((8, 16, 32, 64, 128)[k % 5])
    rng = np.random.default_rng(C * HW)
    pred = rng.standard_normal((B, C, HW)).astype(f32)
    centres = (rng.integers(0, 1400, (B, HW, 2)) * 1.0).astype(f32)
    out, dpred, dcen = _out(B * HW * C), _dev(pred), _dev(centres)
    lib.check(L.kgdet_pts_from_offsets_forward(_ptr(dpred), _ptr(dcen), out.ptr(), c_i64(B), c_i32(C), c_i64(HW), c_f(stride),
                                               c_i32(y_first), _st()), 'pts_from_offsets_forward')
    assert out.intact() and _np_bits_equal(out.view().cpu().numpy().reshape(B, HW, C), R.pts_from_offsets_f32(pred, centres, stride, y_first))
    g = rng.standard_normal((B, HW, C)).astype(f32)
    gp, dg = _out(B * C * HW), _dev(g)
    lib.check(L.kgdet_pts_from_offsets_backward(_ptr(dg), gp.ptr(), c_i64(B), c_i32(C), c_i64(HW), c_f(stride), c_i32(y_first), _st()),
              'pts_from_offsets_backward')
    assert gp.intact() and _np_bits_equal(gp.view().cpu().numpy().reshape(B, C, HW), R.pts_from_offsets_grad_f32(g, stride, y_first))


def test_pts_from_offsets_refuses_an_odd_channel_count():
    lib, L = _L()
    a, out = torch.zeros(64, device='cuda'), Guarded(64)
    assert L.kgdet_pts_from_offsets_forward(_ptr(a), _ptr(a), out.ptr(), c_i64(1), c_i32(3), c_i64(4), c_f(8.0), c_i32(1), _st()) == E_SHAPE
    assert L.kgdet_pts_from_offsets_backward(_ptr(a), out.ptr(), c_i64(1), c_i32(3), c_i64(4), c_f(8.0), c_i32(1), _st()) == E_SHAPE
    torch.cuda.synchronize()
    assert (out.buf == CANARY).all()


# ============================================================================================ inference epilogues
class GuardedT(object):
    """a CPU tensor of any dtype as the payload of a device buffer of 777 (64 elements either side)"""

    def __init__(self, t):
        self.n = t.numel()
        self.buf = torch.full((64 + self.n + 64,), 777.0, dtype=t.dtype, device='cuda')
        self.view().copy_(t.reshape(-1))

    def view(self):
        return self.buf[64:64 + self.n]

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 64 * self.buf.element_size())

    def intact(self):
        return bool((self.buf[:64] == 777.0).all()) and bool((self.buf[64 + self.n:] == 777.0).all())


def _same_bits(a, b):
    a, b = a.contiguous().reshape(-1).cpu(), b.contiguous().reshape(-1).cpu()
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.dtype == b.dtype and bool(torch.equal(a.view(it), b.view(it)))


DTYPES = [(0, torch.float32), (1, torch.bfloat16)]
FLAGS = [(res, relu, bias) for res in (0, 1) for relu in (0, 1) for bias in (0, 1)]


def _bias_act_case(N, C, HW, code, dtype, channels_last, flags, seed=0):
    lib, L = _L()
    gen = torch.Generator().manual_seed(seed + N * C + HW)
    shape = (N, HW, C) if channels_last else (N, C, HW)
    x0 = (torch.randn(shape, generator=gen) * 3).to(dtype)
    r0 = torch.randn(shape, generator=gen).to(dtype)
    b0 = torch.randn(C, generator=gen)
    rd, bd = r0.cuda(), b0.cuda()
    for res, relu, bias in flags:
        x = GuardedT(x0)
        lib.check(L.kgdet_bias_act(x.ptr(), _ptr(bd if bias else None), ctypes.c_void_p(rd.data_ptr() if res else 0), c_i64(N), c_i32(C),
                                   c_i64(HW), c_i32(code), c_i32(relu), c_i32(int(channels_last)), _st()), 'bias_act')
        want = R.bias_act_restated(x0, b0 if bias else None, r0 if res else None, relu, channels_last)
        assert x.intact(), (res, relu, bias)
        assert _same_bits(x.view(), want), (res, relu, bias)


@pytest.mark.parametrize('code,dtype', DTYPES)
@pytest.mark.parametrize('N,C,HW', [(3, 5, 1), (2, 6, 7), (2, 8, 35), (2, 16, 1050), (1, 4, 16800)])
def test_bias_act_nchw_bit_exact(N, C, HW, code, dtype):
    """every combination of residual, ReLU and bias (null included); HW = 1, 7, 35, 1050 are not multiples of the vector width of
    either type (the scalar path)"""
    _bias_act_case(N, C, HW, code, dtype, False, FLAGS)


@pytest.mark.parametrize('code,dtype', DTYPES)
@pytest.mark.parametrize('N,C,HW,flags', [(1, 2, 268800, [(1, 1, 1), (0, 0, 0)]), (3, 1500, 7, [(1, 1, 1)]), (3, 1500, 8, [(0, 1, 1)])])
def test_bias_act_nchw_loops_that_wrap(N, C, HW, flags, code, dtype):
    """HW / V beyond 64 x 256 vectors (the inner grid-stride loop) and 4500 planes (the loop over gridDim.y = 4096)"""
    _bias_act_case(N, C, HW, code, dtype, False, flags)


@pytest.mark.parametrize('code,dtype,N,C,HW', [(c, t, N, C, HW) for c, t in DTYPES for N, C, HW in [(2, 4, 35), (2, 8, 35), (1, 64, 130), (1, 2048, 7)]
                                               if C % (4 if c == 0 else 8) == 0])
def test_bias_act_channels_last_bit_exact(code, dtype, N, C, HW):
    """C = 4 (float32 only: a bf16 vector holds 8 channels, see the refusal below), 8, 64, 2048"""
    _bias_act_case(N, C, HW, code, dtype, True, FLAGS)


@pytest.mark.parametrize('code,dtype,N,HW', [(0, torch.float32, 2, 400000), (1, torch.bfloat16, 2, 750000)])
def test_bias_act_channels_last_channel_tracking_over_many_wraps(code, dtype, N, HW):
    """C = 24: 6 / 3 vectors per pixel, which does not divide the capped grid's step of 16384 x 256 vectors -- the incremental
    channel index moves and wraps on every trip (a power-of-two C never moves it); 4.8 M / 4.5 M vectors: two trips"""
    assert N * HW * 24 // (4 if code == 0 else 8) > 16384 * 256
    _bias_act_case(N, 24, HW, code, dtype, True, [(1, 1, 1)])


@pytest.mark.parametrize('code,dtype,C', [(0, torch.float32, 6), (1, torch.bfloat16, 12), (1, torch.bfloat16, 4)])
def test_bias_act_channels_last_refuses_a_ragged_channel_count(code, dtype, C):
    lib, L = _L()
    x0 = torch.randn(2, 5, C).to(dtype)
    x, b = GuardedT(x0), torch.randn(C).cuda()
    assert L.kgdet_bias_act(x.ptr(), _ptr(b), None, c_i64(2), c_i32(C), c_i64(5), c_i32(code), c_i32(1), c_i32(1), _st()) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert x.intact() and _same_bits(x.view(), x0)


@pytest.mark.parametrize('code,dtype', DTYPES)
@pytest.mark.parametrize('N,H,W,C', [(2, 1, 1, 8), (2, 2, 2, 8), (2, 7, 9, 16), (1, 400, 672, 8)])
def test_bias_relu_maxpool_nhwc_bit_exact(N, H, W, C, code, dtype):
    """both instantiations, 1 x 1, 2 x 2 and odd maps, with and without a bias; inputs all negative after the bias give exactly 0
    (the zero the maximum starts from is relu's floor, not leaked padding)"""
    lib, L = _L()
    gen = torch.Generator().manual_seed(H * W)
    x0 = torch.randn((N, H, W, C), generator=gen).to(dtype)
    b0 = torch.randn(C, generator=gen)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    for xin, bias in ((x0, b0), (x0, None), (-x0.abs() - 0.5, -b0.abs())):
        y = GuardedT(torch.full((N, Ho, Wo, C), NAN).to(dtype))
        xd, bd = xin.cuda(), (None if bias is None else bias.cuda())
        lib.check(L.kgdet_bias_relu_maxpool_nhwc(ctypes.c_void_p(xd.data_ptr()), _ptr(bd), y.ptr(), c_i64(N), c_i32(C), c_i32(H), c_i32(W),
                                                 c_i32(code), _st()), 'bias_relu_maxpool_nhwc')
        want = R.bias_relu_maxpool_restated(xin, None if bias is None else bias.numpy())
        assert y.intact() and _same_bits(y.view(), want)
        if bias is not None and bool((bias <= 0).all()):
            assert bool((y.view().float() == 0).all())


# ============================================================================================ frozen BatchNorm (+ add) (+ ReLU)
def _bn_forward(d, res, relu, N, C, HW, gamma=True, beta=True):
    lib, L = _L()
    y = _out(N * C * HW)
    lib.check(L.kgdet_bn_act_forward(_ptr(d['x']), _ptr(d['gamma'] if gamma else None), _ptr(d['beta'] if beta else None), _ptr(d['mean']),
                                     _ptr(d['var']), c_f(R.BN_EPS), _ptr(d['res'] if res else None), y.ptr(), c_i64(N), c_i32(C), c_i64(HW),
                                     c_i32(relu), _st()), 'bn_act_forward')
    assert y.intact()
    return y


def _bn_backward(d, y, res, relu, N, C, HW, P, gamma=True, beta=True, want_gx=True, with_sums=True):
    lib, L = _L()
    outs = []
    for _ in range(2):
        gx, gr, partial, sums = _out(N * C * HW), _out(N * C * HW), _out(2 * C * P), _out(2 * C)
        lib.check(L.kgdet_bn_act_backward(_ptr(d['gy']), _ptr(d['x']), y.ptr(), _ptr(d['gamma'] if gamma else None),
                                          _ptr(d['beta'] if beta else None), _ptr(d['mean']), _ptr(d['var']), c_f(R.BN_EPS), c_i32(res),
                                          c_i32(relu), gx.ptr() if want_gx else None, gr.ptr(), partial.ptr(),
                                          sums.ptr() if with_sums else None, c_i64(N), c_i32(C), c_i64(HW), _st()), 'bn_act_backward')
        assert gx.intact() and gr.intact() and partial.intact() and sums.intact()
        outs.append([g.view().clone() for g in (gx, gr, partial, sums)])
    for a, b in zip(*outs):
        assert _bit_equal(a, b)
    return [a.cpu().numpy() for a in outs[0]]


def _bn_case(N, C, HW, res, relu, gamma=True, beta=True, want_gx=True, with_sums=True):
    lib, L = _L()
    h = R.bn_inputs(N, C, HW)
    d = {k: _dev(v) for k, v in h.items()}
    chunks, per, P = R.bn_chunks(N, C, HW)
    assert L.kgdet_bn_act_partials(c_i64(N), c_i32(C), c_i64(HW)) == P
    hg, hb = (h['gamma'] if gamma else None), (h['beta'] if beta else None)
    tag = 'bn_act N%d C%d HW%d res%d relu%d: ' % (N, C, HW, res, relu)
    y = _bn_forward(d, res, relu, N, C, HW, gamma, beta)
    got_y = y.view().cpu().numpy().reshape(N, C, HW)
    want_y, pre, bound = R.bn_act_forward(h['x'], hg, hb, h['mean'], h['var'], R.BN_EPS, h['res'] if res else None, relu)
    assert _ratio(got_y, want_y, bound, tag + 'y') <= 1.0
    mask = None
    if relu:       # the kernel's mask is the float64 one outside the window the forward bound leaves around zero: few elements
        window = R.relu_window(pre, bound)
        assert window.sum() <= 1e-3 * pre.size
        mask = got_y > 0
        assert ((mask == (pre > 0)) | window).all() and (got_y >= 0).all()
    gx, gr, partial, sums = _bn_backward(d, y, res, relu, N, C, HW, P, gamma, beta, want_gx, with_sums)
    ref = R.bn_act_backward(h['gy'], h['x'], hg, hb, h['mean'], h['var'], R.BN_EPS, mask)
    if want_gx:
        assert _ratio(gx.reshape(N, C, HW), ref['grad_x'], ref['bound_x'], tag + 'grad_x') <= 1.0
        if relu:      # the backward's mask IS the forward's, element for element (the gradients below are never 0)
            assert ((gx.reshape(N, C, HW) != 0) == (mask & (h['gy'] != 0))).all()
    else:
        assert np.isnan(gx).all()
    if res and relu:
        assert _np_bits_equal(gr.reshape(N, C, HW), np.where(mask, h['gy'], f32(0)))
    else:
        assert np.isnan(gr).all()          # not written: the residual's gradient is grad_y itself
    # the partial sums, slot by slot ([2][C][P], slot n * chunks + k): the chain of one workgroup (pointwise_refs.bn_act_chain); a
    # term g (x - mean) has two roundings of its own, the factor invstd three and one product
    L1 = R.bn_act_chain(per)
    s1, a1 = R.chunk_sums(ref['gp'], chunks, per)
    s2, a2 = R.chunk_sums(ref['gxm'], chunks, per)
    partial = partial.reshape(2, C, P)
    assert np.isfinite(partial).all()
    assert _ratio(partial[0], s1, L1 * U * a1, tag + 'partial grad_beta') <= 1.0
    assert _ratio(partial[1], s2, (L1 + 6) * U * a2, tag + 'partial grad_gamma') <= 1.0
    empty = np.arange(chunks) * per >= HW
    assert (partial[:, :, np.tile(empty, N)] == 0).all()
    if with_sums:      # + the P partials added in slot order
        sums = sums.reshape(2, C)
        rb = _ratio(sums[0], ref['grad_beta'], (L1 + P) * U * a1.sum(1), tag + 'grad_beta')
        rg = _ratio(sums[1], ref['grad_gamma'], (L1 + 6 + P) * U * a2.sum(1), tag + 'grad_gamma')
        assert rb <= 1.0 and rg <= 1.0
    else:
        assert np.isnan(sums).all()
    return chunks, per


@pytest.mark.parametrize('res,relu', [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize('N,C,HW', R.BN_SHAPES)
def test_bn_act_against_float64(N, C, HW, res, relu):
    """the shapes of test_frozen_bn_act_matches_torch, HW = 1, 3, 4, 5 and 1023 .. 1025 (the vector and the scalar path, one and two
    chunks), HW = 350300 on 12 planes (342 chunks of 1028 elements: the last chunk is empty) and 40 chunks per plane"""
    chunks, per = _bn_case(N, C, HW, res, relu)
    if HW == 350300:
        assert (chunks - 1) * per >= HW


@pytest.mark.parametrize('gamma,beta,want_gx,with_sums', [(False, False, True, True), (True, False, False, True), (False, True, True, False)])
@pytest.mark.parametrize('N,C,HW', [(2, 37, 1050), (2, 9, 1025)])
def test_bn_act_null_arguments(N, C, HW, gamma, beta, want_gx, with_sums):
    _bn_case(N, C, HW, 1, 1, gamma, beta, want_gx, with_sums)
    _bn_case(N, C, HW, 0, 1, gamma, beta, want_gx, with_sums)


@pytest.mark.parametrize('res', [0, 1])
@pytest.mark.parametrize('n', [4096, 4095])
def test_bn_act_backward_mask_is_the_forward_mask_at_zero(n, res):
    """x s + t lands at 0 and within an ulp or two either side of it (pointwise_refs.bn_near_zero_inputs), through the vector path and
    the scalar one.  Without a residual the backward recomputes the pre-activation: whatever the compiler contracts, the set where the
    forward gave y > 0 must be the set that passes a gradient.  Nothing is left out here."""
    h, s = R.bn_near_zero_inputs(4096)
    h = {k: (np.ascontiguousarray(v[..., :n]) if v.ndim == 3 else v) for k, v in h.items()}
    d = {k: _dev(v) for k, v in h.items()}
    y = _bn_forward(d, res, 1, 1, 2, n)
    got_y = y.view().cpu().numpy().reshape(2, n)
    assert ((got_y == 0).sum(1) > 1000).all() and ((got_y > 0).sum(1) > 700).all()
    if not res:
        assert (got_y[1, ::4] == 0).all()          # channel 1: x s + t is exactly 0 there
    gx, gr, partial, sums = _bn_backward(d, y, res, 1, 1, 2, n, R.bn_chunks(1, 2, n)[2])
    assert ((gx.reshape(2, n) != 0) == (got_y > 0)).all()
    if res:
        assert ((gr.reshape(2, n) != 0) == (got_y > 0)).all()


def test_bn_act_refuses_65536_planes():
    lib, L = _L()
    a = torch.zeros(65536, device='cuda')
    out, part = Guarded(65536), Guarded(64)
    args = (c_i64(2), c_i32(32768), c_i64(1), _st())
    assert L.kgdet_bn_act_forward(_ptr(a), None, None, _ptr(a), _ptr(a), c_f(1e-5), None, out.ptr(), c_i64(2), c_i32(32768), c_i64(1),
                                  c_i32(1), _st()) == E_SHAPE
    assert L.kgdet_bn_act_backward(_ptr(a), _ptr(a), None, None, None, _ptr(a), _ptr(a), c_f(1e-5), c_i32(0), c_i32(1), out.ptr(), None,
                                   part.ptr(), None, *args) == E_SHAPE
    assert L.kgdet_bn_fold_backward(_ptr(a), _ptr(a), c_i32(1), out.ptr(), part.ptr(), *args) == E_SHAPE
    torch.cuda.synchronize()
    assert (out.buf == CANARY).all() and (part.buf == CANARY).all()


@pytest.mark.parametrize('N,C,H,W', [(2, 5, 1, 1), (2, 5, 7, 9), (1, 3, 13, 8), (2, 4, 51, 85), (1, 2, 2, 2)])
def test_bn_relu_maxpool_against_float64(N, C, H, W):
    lib, L = _L()
    h = R.bn_inputs(N, C, H * W, seed=3)
    want, bound = R.bn_relu_maxpool(h['x'].reshape(N, C, H, W), h['gamma'], h['beta'], h['mean'], h['var'], R.BN_EPS)
    d = {k: _dev(v) for k, v in h.items()}
    y = _out(want.size)
    lib.check(L.kgdet_bn_relu_maxpool(_ptr(d['x']), _ptr(d['gamma']), _ptr(d['beta']), _ptr(d['mean']), _ptr(d['var']), c_f(R.BN_EPS), y.ptr(),
                                      c_i64(N), c_i32(C), c_i32(H), c_i32(W), _st()), 'bn_relu_maxpool')
    got = y.view().cpu().numpy().reshape(want.shape)
    assert y.intact() and (got >= 0).all()
    assert _ratio(got, want, bound, 'bn_relu_maxpool %dx%d' % (H, W)) <= 1.0


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('HW', [1050, 1051, 1053, 3, 16800])
def test_bn_fold_backward(HW, relu):
    """g = grad_z * [z > 0] bit-exact (z holds exact zeros and negative zeros), written only with relu; the per-workgroup sums [C][P]
    inside the chain of relu_sum_bwd_kernel; HW = 1051, 1053, 3: the ragged tail after the unaligned vector loop"""
    lib, L = _L()
    N, C = 2, 5
    rng = np.random.default_rng(HW)
    gz = rng.standard_normal((N, C, HW)).astype(f32)
    z = np.maximum(rng.standard_normal((N, C, HW)), 0).astype(f32)
    z[:, :, ::7] = -0.0
    chunks, per, P = R.bn_chunks(N, C, HW)
    g, partial, dgz, dz = _out(N * C * HW), _out(C * P), _dev(gz), _dev(z)
    lib.check(L.kgdet_bn_fold_backward(_ptr(dgz), _ptr(dz), c_i32(relu), g.ptr(), partial.ptr(), c_i64(N), c_i32(C), c_i64(HW),
                                       _st()), 'bn_fold_backward')
    assert g.intact() and partial.intact()
    want = np.where(z > 0, gz, f32(0)) if relu else gz
    if relu:
        assert _np_bits_equal(g.view().cpu().numpy().reshape(N, C, HW), want)
    else:
        assert bool(torch.isnan(g.view()).all())
    s, a = R.chunk_sums(want.astype(np.float64), chunks, per)
    r = _ratio(partial.view().cpu().numpy().reshape(C, P), s, R.bn_fold_chain(per) * U * a, 'bn_fold_backward HW%d relu%d partial' % (HW, relu))
    assert r <= 1.0


def test_bn_fold_finish_against_the_float64_definition():
    """grad_gamma from the <w, G> identity against invstd sum g' (y - mean) of a small real convolution evaluated in float64
    (pointwise_refs.fold_case); G scaled by s in place; G == NULL: grad_beta alone, and with grad_gamma set the refusal"""
    lib, L = _L()
    c = R.fold_case()
    O, CK = c['w'].shape
    P = c['partial'].shape[1]
    r = R.bn_fold_finish(c['partial'], c['w'], c['G'], c['s'], c['mean'], c['var'], R.BN_EPS)
    slack = R.fold_input_slack(c)
    d = {k: _dev(c[k]) for k in ('partial', 'w', 's', 'mean', 'var')}

    def call(G, gb, gg):
        return L.kgdet_bn_fold_finish(_ptr(d['partial']), c_i32(P), _ptr(d['w']), G.ptr() if G else None, _ptr(d['s']), _ptr(d['mean']),
                                      _ptr(d['var']), c_f(R.BN_EPS), gb.ptr() if gb else None, gg.ptr() if gg else None, c_i32(O), c_i32(CK), _st())
    G, gb, gg = Guarded(O * CK, fill=c['G']), _out(O), _out(O)
    assert call(G, gb, gg) == 0
    assert G.intact() and gb.intact() and gg.intact()
    rb = _ratio(gb.view().cpu().numpy(), c['want_beta'], r['bound_beta'] + slack['beta'], 'bn_fold_finish grad_beta')
    rg = _ratio(gg.view().cpu().numpy(), c['want_gamma'], r['bound_gamma'] + slack['gamma'], 'bn_fold_finish grad_gamma')
    assert rb <= 1.0 and rg <= 1.0
    assert _np_bits_equal(G.view().cpu().numpy().reshape(O, CK), c['G'] * c['s'][:, None])          # one product: bit-exact
    gb2, gg2 = _out(O), _out(O)
    assert call(None, gb2, None) == 0
    assert _bit_equal(gb2.view(), gb.view()) and bool(torch.isnan(gg2.view()).all())
    gb3 = _out(O)
    assert call(None, gb3, gg2) == E_SHAPE
    torch.cuda.synchronize()
    assert bool(torch.isnan(gb3.view()).all()) and bool(torch.isnan(gg2.view()).all())
