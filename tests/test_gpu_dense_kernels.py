"""The dense convolutions -- csrc/dense_forward.hip, dense_grad_weight.hip -- through the C ABI against tests/dense_refs.py, one
case per branch of plan_nn / plan_gw.  Every test first asks the library which plan its shape takes (kgdet_conv_apply_plan,
kgdet_conv_grad_weight_plan) and fails if that is not the branch the case is named for: a cost model that moves must move the
table with it.  Then three tiers (dense_refs.py):

  exact         lattice operands: the bits of S3, in bf16 and fp16 parts, twice, the workspace prefilled with NaN and with large
                finite garbage, outputs prefilled with NaN inside canaries;
  accumulation  mixed-scale operands: |got - S3| <= ACC_BAR * max |ref| per output channel / weight-gradient row / image;
  envelope      bf16 backward results at gradient magnitude: 1e-5 per group against the exact float64 result (where the split
                itself leaves room: dense_refs.BF16_SPLIT_OVER).

The largest ratio of every case is printed before it is asserted.
"""
import numpy as np
import pytest
import torch

from tests import dense_refs as R
from tests.test_gpu_step_kernels import CANARY, Guarded

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN = float('nan')
GARBAGE = 1e30
E_SHAPE = 1
U = 2.0 ** -24
FMTS = [R.BF16, R.FP16]
BN_EPS = 1e-5


def _L():
    from kgdet_amd import _lib, conv1x1
    return _lib, conv1x1._library()


def _st():
    from kgdet_amd import _lib
    return _lib.raw_stream()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, f32)).cuda()


def _p(t):
    """device address of a tensor, a Guarded payload or NULL"""
    if t is None:
        return None
    if isinstance(t, Guarded):
        return t.buf.data_ptr() + 4 * t.lead
    return t.data_ptr()


def _out(n, fill=NAN):
    g = Guarded(max(int(n), 1))
    g.view().fill_(fill)
    return g


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.int32)


def _same_bits(got, ref64, tag):
    ref = np.asarray(ref64, np.float64)
    ref32 = ref.astype(f32)
    assert (ref32.astype(np.float64) == ref).all(), tag + ': the reference is no float32 number'
    bad = _bits(got.reshape(ref.shape)) != _bits(ref32)
    assert not bad.any(), '%s: %d of %d elements differ, first at %s: got %r, want %r' % (
        tag, int(bad.sum()), bad.size, np.argwhere(bad)[0], got.reshape(ref.shape)[tuple(np.argwhere(bad)[0])], ref32[tuple(np.argwhere(bad)[0])])


def _measure(got, ref, axis, bar, tag):
    r = R.group_ratio(got, ref, axis)
    print('%s: %.3g per group, %.3f of its bar' % (tag, r, r / bar))
    return r


# ============================================================================================ packers
def _pack(w, taps, transpose, fmt):
    """kgdet_conv_pack_fmt of w [O, C, k, k] -> the image, inside canaries"""
    lib, L = _L()
    O, C = w.shape[0], w.shape[1]
    M, K = (C, O) if transpose else (O, C)
    nbytes = L.kgdet_conv_packed_bytes(M, K, taps)
    assert nbytes > 0 and nbytes % 4 == 0
    img, dw = _out(nbytes // 4), _dev(w)
    lib.check(L.kgdet_conv_pack_fmt(_p(dw), O, C, taps, transpose, _p(img), fmt, _st()), 'conv_pack_fmt')
    assert img.intact()
    return img


def _image_matrix(img, M, K, T, f16):
    """the image [mt][k16 * T + t][part][khalf][128][8] as float32 [part][rows][reduction][tap], rows and reduction padded"""
    u = img.view().cpu().numpy().view(np.uint16)
    n_mt, k16s = -(-M // 128), -(-K // 16)
    u = u.reshape(n_mt, k16s, T, 2, 2, 128, 8)
    v = u.view(np.float16).astype(f32) if f16 else (u.astype(np.uint32) << 16).view(f32)
    return v.transpose(3, 0, 5, 1, 4, 6, 2).reshape(2, n_mt * 128, k16s * 16, T)


PACK_SHAPES = [(130, 48, 1), (33, 13, 1), (64, 32, 9), (96, 144, 9)]


@pytest.mark.parametrize('O,C,taps', PACK_SHAPES)
def test_packers_agree_and_hold_the_restated_split(O, C, taps):
    """kgdet_conv_pack_fmt, _both_fmt and _multi write the same images; the images are the restated parts (fp16: of w x 2^8) with the
    grad_input image's taps mirrored and zeros up to the tile; _multi with a power-of-two scale per output channel packs w x s"""
    lib, L = _L()
    k = 3 if taps == 9 else 1
    rng = np.random.default_rng(O + C)
    w = (0.1 * rng.standard_normal((O, C, k, k)) * 10.0 ** rng.uniform(-4, 1, (O, 1, 1, 1))).astype(f32)
    w[0, 0] = 300.0                                          # fp16 parts: beyond the image's range, saturated
    s = (2.0 ** rng.integers(-6, 4, O)).astype(f32)
    s[O // 2] = 0.0
    dw, ds = _dev(w), _dev(s)
    nb, nbt = L.kgdet_conv_packed_bytes(O, C, taps), L.kgdet_conv_packed_bytes(C, O, taps)
    both_ok = taps == 1 or (O % 16 == 0 and C % 16 == 0)
    for fmt in FMTS:
        single, single_t = _pack(w, taps, 0, fmt), (_pack(w, taps, 1, R.BF16) if taps == 1 or O % 16 == 0 else None)
        # the restatement
        for img, M, K, f16, tr in ((single, O, C, fmt == R.FP16, False), (single_t, C, O, False, True)):
            if img is None:
                continue
            A = w.reshape(O, C, taps)
            A = A.transpose(1, 0, 2)[:, :, ::-1] if tr else A
            hi, lo, _ = R.split_weight(np.ascontiguousarray(A), R.FP16 if f16 else R.BF16)
            want = np.zeros((2, -(-M // 128) * 128, -(-K // 16) * 16, taps), f32)
            want[0, :M, :K], want[1, :M, :K] = hi.numpy(), lo.numpy()
            got = _image_matrix(img, M, K, taps, f16)
            assert (_bits(got) == _bits(want)).all() or (got == want).all(), (fmt, tr)     # (+0 / -0 padding counts as equal)
        if not both_ok:
            continue
        a, at = _out(nb // 4), _out(nbt // 4)
        lib.check(L.kgdet_conv_pack_both_fmt(_p(dw), O, C, taps, _p(a), _p(at), fmt, _st()), 'conv_pack_both_fmt')
        assert a.intact() and at.intact()
        assert torch.equal(a.view().view(torch.int32), single.view().view(torch.int32))
        assert torch.equal(at.view().view(torch.int32), single_t.view().view(torch.int32))
        # multi: two descriptors, the second with the scale
        m0, m0t, m1, m1t = _out(nb // 4), _out(nbt // 4), _out(nb // 4), _out(nbt // 4)
        blocks = L.kgdet_conv_pack_blocks(O, C, taps)
        f16bit = (1 << 62) if fmt == R.FP16 else 0
        desc = torch.tensor([[_p(dw), _p(m0), _p(m0t), (O << 32) | C, (taps << 32) | 0 | f16bit, 0],
                             [_p(dw), _p(m1), _p(m1t), (O << 32) | C, (taps << 32) | blocks | f16bit, _p(ds)]], dtype=torch.int64).cuda()
        lib.check(L.kgdet_conv_pack_multi(desc.data_ptr(), 2, 2 * blocks, _st()), 'conv_pack_multi')
        for g in (m0, m0t, m1, m1t):
            assert g.intact()
        assert torch.equal(m0.view().view(torch.int32), single.view().view(torch.int32))
        assert torch.equal(m0t.view().view(torch.int32), single_t.view().view(torch.int32))
        ws = (w * s.reshape(O, 1, 1, 1)).astype(f32)
        assert torch.equal(m1.view().view(torch.int32), _pack(ws, taps, 0, fmt).view().view(torch.int32))
        assert torch.equal(m1t.view().view(torch.int32), _pack(ws, taps, 1, R.BF16).view().view(torch.int32))


# ============================================================================================ forward and stride-1 grad_input
PLAN_WORDS = 11


def _fwd_plan(c):
    lib, L = _L()
    out = torch.zeros(PLAN_WORDS + 2, dtype=torch.int32)
    out[PLAN_WORDS:] = 77
    lib.check(L.kgdet_conv_apply_plan(c.B, c.M, c.K, c.H, c.W, c.taps, c.stride, out.data_ptr()), 'conv_apply_plan')
    assert out[PLAN_WORDS:].tolist() == [77, 77]
    return out[:PLAN_WORDS].tolist()


def _assert_fwd_plan(c):
    plan = _fwd_plan(c)
    got = (R.fwd_kernel_of(plan, c.taps), plan[5], plan[9])
    assert got == (c.kernel, c.ks, c.closer), '%s takes %s, not the branch it is named for (%s)' % (c.name, got, (c.kernel, c.ks, c.closer))
    assert plan[10] == (3 if c.ks > 1 else 0)
    lib, L = _L()
    Ho, Wo = -(-c.H // c.stride), -(-c.W // c.stride)
    assert L.kgdet_conv_apply_workspace_bytes(c.B, c.M, c.K, c.H, c.W, c.taps, c.stride) == (4 * c.ks * c.B * c.M * Ho * Wo if c.ks > 1 else 0)
    return plan


def _apply(c, img, x, fmt, bias=None, residual=None, relu=0, gate=None, ws_fill=NAN):
    """kgdet_conv_apply_gated_fmt -> (status, y [B, M, Ho, Wo]); output and workspace inside canaries"""
    lib, L = _L()
    Ho, Wo = -(-c.H // c.stride), -(-c.W // c.stride)
    wsb = L.kgdet_conv_apply_workspace_bytes(c.B, c.M, c.K, c.H, c.W, c.taps, c.stride)
    y, ws = _out(c.B * c.M * Ho * Wo), _out(wsb // 4, ws_fill)
    rc = L.kgdet_conv_apply_gated_fmt(_p(img), _p(x), _p(y), _p(bias), _p(residual), relu, _p(gate), c.B, c.M, c.K, c.H, c.W, c.taps,
                                      c.stride, fmt, _p(ws), wsb, _st())
    torch.cuda.synchronize()
    assert y.intact() and ws.intact() and img.intact(), c.name
    return rc, y.view().cpu().numpy().reshape(c.B, c.M, Ho, Wo)


def _fwd_params():
    return [pytest.param(c.name, fmt, id='%s-fmt%d' % (c.name, fmt)) for c in R.FWD_CASES for fmt in ([R.BF16] if c.transpose else FMTS)]


@pytest.mark.parametrize('name,fmt', _fwd_params())
def test_forward_branch(name, fmt):
    """exact: plain and with the whole epilogue (bias, residual, ReLU; the gate where the ABI takes one), workspace NaN and garbage.
    accumulation: mixed-scale weight rows (grad_input cases: gradient-sized images), against S3 per output channel (image).
    envelope (grad_input cases): 1e-5 per image against the exact float64 result."""
    lib, L = _L()
    c = R.FWD_BY_NAME[name]
    plan = _assert_fwd_plan(c)
    if 'uneven' in name:
        assert (c.taps * -(-c.K // 16)) % c.ks != 0
    op, k = R.fwd_op(c), (3 if c.taps == 9 else 1)
    la = R.fwd_lattice(name, fmt)
    conv = R.s3(op, la.a, la.b, fmt).numpy()
    img, x = _pack(la.b, c.taps, 1 if c.transpose else 0, fmt), _dev(la.a)
    bias, residual, gate = _dev(la.bias), _dev(la.residual), _dev(la.gate)
    gated = c.closer != 2
    full = R.epilogue(conv, la.bias, la.residual, True, la.gate if gated else None)
    for fill in (NAN, GARBAGE):
        rc, y = _apply(c, img, x, fmt, ws_fill=fill)
        lib.check(rc, 'conv_apply')
        _same_bits(y, conv + 0.0, '%s fmt%d plain' % (name, fmt))
        rc, y = _apply(c, img, x, fmt, bias, residual, 1, gate if gated else None, ws_fill=fill)
        lib.check(rc, 'conv_apply')
        _same_bits(y, full, '%s fmt%d epilogue' % (name, fmt))
    # accumulation
    xm, wm = R.fwd_mixed(name)
    axis = 0 if c.transpose else 1
    s3 = R.s3(op, xm, wm, fmt).numpy()
    rc, y = _apply(c, _pack(wm, c.taps, 1 if c.transpose else 0, fmt), _dev(xm), fmt)
    lib.check(rc, 'conv_apply')
    tag = 'forward %s fmt%d (%s ks %d)' % (name, fmt, c.kernel, c.ks)
    r = _measure(y, s3, axis, R.ACC_BAR, tag + ' accumulation')
    assert r <= R.ACC_BAR, tag
    if c.transpose:
        ex = R.exact(op, xm, wm).numpy()
        assert _measure(y, ex, 0, R.SPLIT_BAR[R.BF16], tag + ' envelope') <= R.SPLIT_BAR[R.BF16], tag


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('name', R.CLOSER_CASES)
def test_closing_passes(name, fmt):
    """bias, residual, ReLU and gate in every combination on each closing pass: the kernel's store (ks == 1), conv1x1_sum_epilogue
    (even pixel count), conv1x1_sum + kgdet_bias_act (odd pixel count, where a gate is refused and nothing is written)"""
    lib, L = _L()
    c = R.FWD_BY_NAME[name]
    _assert_fwd_plan(c)
    la = R.fwd_lattice(name, fmt)
    conv = R.s3(R.fwd_op(c), la.a, la.b, fmt).numpy()
    img, x = _pack(la.b, c.taps, 0, fmt), _dev(la.a)
    dev = dict(bias=_dev(la.bias), residual=_dev(la.residual), gate=_dev(la.gate))
    for mask in range(16):
        use = dict(bias=mask & 1, residual=mask & 2, relu=mask & 4, gate=mask & 8)
        args = {k2: (dev[k2] if use[k2] else None) for k2 in dev}
        rc, y = _apply(c, img, x, fmt, args['bias'], args['residual'], 1 if use['relu'] else 0, args['gate'], ws_fill=GARBAGE if mask & 1 else NAN)
        if c.closer == 2 and use['gate']:
            assert rc == E_SHAPE and np.isnan(y).all(), (name, mask)
            continue
        lib.check(rc, 'conv_apply')
        ref = R.epilogue(conv, la.bias if use['bias'] else None, la.residual if use['residual'] else None, bool(use['relu']),
                         la.gate if use['gate'] else None)
        _same_bits(y, ref, '%s fmt%d flags %d' % (name, fmt, mask))


@pytest.mark.parametrize('fmt', FMTS)
def test_fp16_forward_small_weight_rows(fmt):
    """The envelope of the forward parts per output channel (nn1_ks2_uneven's mixed-scale weights: rows from 1e-5 to 1): the kernel stays
    inside the accumulation bar of S3 on EVERY row, i.e. it gives what the format can give -- which for fp16 parts is the documented
    1e-6 only on rows whose weights stay above ~2^-11 (tests/test_dense_refs.py measures S3 - exact per row: 6e-6 at 1e-5)."""
    lib, L = _L()
    c = R.FWD_BY_NAME['nn1_ks2_uneven']
    x, w = R.fwd_mixed(c.name)
    op = R.fwd_op(c)
    s3, ex = R.s3(op, x, w, fmt).numpy(), R.exact(op, x, w).numpy()
    rc, y = _apply(c, _pack(w, c.taps, 0, fmt), _dev(x), fmt)
    lib.check(rc, 'conv_apply')
    rms = np.sqrt((w.astype(np.float64) ** 2).mean(axis=(1, 2, 3)))
    inside = rms >= 4 * R.F16_WEIGHT_NORMAL_LO
    assert _measure(y, s3, 1, R.ACC_BAR, 'small rows fmt%d against S3' % fmt) <= R.ACC_BAR
    bar = R.SPLIT_BAR[fmt]
    assert _measure(y[:, inside], ex[:, inside], 1, bar, 'rows inside the envelope fmt%d against float64' % fmt) <= bar + R.ACC_BAR
    _measure(y[:, ~inside], ex[:, ~inside], 1, bar, 'rows below the envelope fmt%d against float64' % fmt)


# ============================================================================================ stride-2 grad_input, stem
@pytest.mark.parametrize('B,C,O,Hin,Win', R.S2GI_CASES)
def test_conv3x3_s2_grad_input(B, C, O, Hin, Win):
    lib, L = _L()
    op = R.op_grad_input(3, 2, Hin, Win)

    def run(gy, w):
        img, dgy, gx = _pack(w, 9, 1, R.BF16), _dev(gy), _out(B * C * Hin * Win)
        lib.check(L.kgdet_conv3x3_s2_grad_input(_p(img), _p(dgy), _p(gx), B, C, O, Hin, Win, _st()), 'conv3x3_s2_grad_input')
        torch.cuda.synchronize()
        assert gx.intact() and img.intact()
        return gx.view().cpu().numpy().reshape(B, C, Hin, Win)

    la = R.s2gi_lattice(B, C, O, Hin, Win)
    ref = R.s3(op, la.a, la.b, R.BF16).numpy() + 0.0
    for _ in range(2):
        _same_bits(run(la.a, la.b), ref, 's2 grad_input %s' % ((B, C, O, Hin, Win),))
    gy, w = R.s2gi_mixed(B, C, O, Hin, Win)
    got = run(gy, w)
    tag = 's2 grad_input %s' % ((B, C, O, Hin, Win),)
    assert _measure(got, R.s3(op, gy, w, R.BF16).numpy(), 0, R.ACC_BAR, tag + ' accumulation') <= R.ACC_BAR
    assert _measure(got, R.exact(op, gy, w).numpy(), 0, R.SPLIT_BAR[R.BF16], tag + ' envelope') <= R.SPLIT_BAR[R.BF16]


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('B,H,W', R.STEM_CASES)
def test_stem_conv7x7_s2(B, H, W, fmt):
    lib, L = _L()
    op = R.op_forward(7, 2)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1

    def run(x, w):
        w160 = np.zeros((64, 160, 1, 1), f32)
        w160[:, :147, 0, 0] = w.reshape(64, 147)
        img, dx, y = _pack(w160, 1, 0, fmt), _dev(x), _out(B * 64 * Ho * Wo)
        lib.check(L.kgdet_stem_conv7x7_s2_fmt(_p(img), _p(dx), _p(y), B, H, W, fmt, _st()), 'stem_conv7x7_s2')
        torch.cuda.synchronize()
        assert y.intact() and img.intact()
        return y.view().cpu().numpy().reshape(B, 64, Ho, Wo)

    la = R.stem_lattice(B, H, W, fmt)
    _same_bits(run(la.a, la.b), R.s3(op, la.a, la.b, fmt).numpy() + 0.0, 'stem %s fmt%d' % ((B, H, W), fmt))
    rng = np.random.default_rng(H * W)
    x, w = rng.standard_normal((B, 3, H, W)).astype(f32), (0.1 * rng.standard_normal((64, 3, 7, 7)) * 10.0 ** rng.uniform(-2, 1, (64, 1, 1, 1))).astype(f32)
    tag = 'stem %s fmt%d accumulation' % ((B, H, W), fmt)
    assert _measure(run(x, w), R.s3(op, x, w, fmt).numpy(), 1, R.ACC_BAR, tag) <= R.ACC_BAR


# ============================================================================================ weight gradients
GW_WORDS = 10


def _gw_plan(c):
    lib, L = _L()
    out = torch.zeros(GW_WORDS + 2, dtype=torch.int32)
    out[GW_WORDS:] = 77
    lib.check(L.kgdet_conv_grad_weight_plan(*(R.gw_plan_args(c) + (out.data_ptr(),))), 'conv_grad_weight_plan')
    assert out[GW_WORDS:].tolist() == [77, 77]
    return out[:GW_WORDS].tolist()


def _gw_run(c, gy, x, closer, gl=None, ws_fill=NAN):
    """one weight gradient through the entry point of its route and closer -> (grad_w [O, C, k, k], grad_beta, grad_gamma)"""
    lib, L = _L()
    k, stride, Ho, Wo = R.gw_geometry(c)
    size = {'1x1': lambda: L.kgdet_conv1x1_grad_weight_workspace_bytes(c.B, c.O, c.C, c.W),
            '3x3': lambda: L.kgdet_conv3x3_grad_weight_workspace_bytes(c.B, c.O, c.C, c.H, c.W),
            's2': lambda: L.kgdet_conv3x3_s2_grad_weight_workspace_bytes(c.B, c.O, c.C, c.H, c.W)}[c.route]()
    assert size > 0 and size % 4 == 0
    ws, gw = _out(size // 4, ws_fill), _out(c.O * c.C * k * k)
    dgy, dx = _dev(gy), _dev(x)
    beta = gamma = None
    head = (_p(dgy), _p(dx), _p(gw), c.B, c.O, c.C) + ((c.W,) if c.route == '1x1' else (c.H, c.W)) + (_p(ws), size)
    if closer in ('fold', 'fold_rows'):
        beta, gamma = _out(c.O), _out(c.O)
        fold = [_dev(t) for t in (gl.w, gl.s, gl.mean, gl.var)]
        bnp = _dev(gl.bn_partial) if closer == 'fold' else None
        tail = tuple(_p(t) for t in fold) + (BN_EPS, _p(bnp), gl.bn_partial.shape[1] if closer == 'fold' else 0, _p(beta), _p(gamma), _st())
        fn = L.kgdet_conv1x1_grad_weight_fold if c.route == '1x1' else L.kgdet_conv3x3_grad_weight_fold
        lib.check(fn(*(head + tail)), 'grad_weight_fold')
    else:
        fn = {'1x1': L.kgdet_conv1x1_grad_weight, '3x3': L.kgdet_conv3x3_grad_weight, 's2': L.kgdet_conv3x3_s2_grad_weight}[c.route]
        lib.check(fn(*(head + (_st(),))), 'grad_weight')
    torch.cuda.synchronize()
    for g in (ws, gw, beta, gamma):
        assert g is None or g.intact(), c.name
    host = lambda g: None if g is None else g.view().cpu().numpy()
    return host(gw).reshape(c.O, c.C, k, k), host(beta), host(gamma)


@pytest.mark.parametrize('name', [c.name for c in R.GW_CASES])
def test_grad_weight_branch(name):
    """exact: every closing pass of the route, twice (workspace NaN, garbage); the folded closer's grad_w = s G and grad_beta exact,
    grad_gamma inside the bound counted from conv_wsum_fold's expression (<= 3 columns per thread, 6 shuffle and 16 serial additions,
    the mean term, the division and the square root: 32 U of the terms' scale).  accumulation and envelope: grad_y channels at
    1e-8 x 10^U(-3, 0), half of the elements masked, per weight-gradient row."""
    c = R.GW_BY_NAME[name]
    plan = _gw_plan(c)
    got = (R.gw_product_of(plan), plan[3])
    assert got == (c.product, c.splits), '%s takes %s, not the branch it is named for (%s)' % (name, got, (c.product, c.splits))
    assert plan[6] == 0 and plan[7] * 256 >= 4 * c.splits * c.O * R.gw_plan_args(c)[2] * R.gw_plan_args(c)[5] and plan[8] >= plan[7]
    op = R.gw_op(c)
    gl = R.gw_lattice(name)
    G = R.s3(op, gl.gy, gl.x, R.BF16).numpy() + 0.0
    for closer in c.closers:
        for fill in (NAN, GARBAGE):
            gw, beta, gamma = _gw_run(c, gl.gy, gl.x, closer, gl, fill)
            tag = 'grad_weight %s %s' % (name, closer)
            if closer in ('sum', 'wsum'):
                _same_bits(gw, G, tag)
                continue
            want_beta = gl.bn_partial.astype(np.float64).sum(1) if closer == 'fold' else gl.gy.astype(np.float64).sum(axis=(0, 2, 3))
            want_gw, want_gamma, scale = R.fold_refs(G, gl, want_beta, BN_EPS)
            _same_bits(gw, want_gw, tag + ' grad_w')          # (the s == 0 row: zeros with the sign of G, as IEEE has them)
            _same_bits(beta, want_beta + 0.0, tag + ' grad_beta')
            err = np.abs(gamma.astype(np.float64) - want_gamma)
            assert (err <= 32 * U * scale).all(), (tag, float((err / np.maximum(32 * U * scale, 1e-300)).max()))
    gy, x = R.gw_mixed(name)
    gw, _, _ = _gw_run(c, gy, x, c.closers[0])
    tag = 'grad_weight %s (%s, %d splits)' % (name, c.product, c.splits)
    assert _measure(gw, R.s3(op, gy, x, R.BF16).numpy(), 0, R.ACC_BAR, tag + ' accumulation') <= R.ACC_BAR, tag
    r = _measure(gw, R.exact(op, gy, x).numpy(), 0, R.SPLIT_BAR[R.BF16], tag + ' envelope')
    assert r <= R.SPLIT_BAR[R.BF16] or name in R.BF16_SPLIT_OVER, tag


def test_plan_queries_refuse_what_the_launch_refuses_and_write_nothing():
    lib, L = _L()
    out = torch.full((16,), 77, dtype=torch.int32)
    for args in ((1, 128, 24, 8, 8, 9, 1), (1, 128, 32, 8, 8, 4, 1), (1, 128, 32, 8, 8, 1, 3), (0, 128, 32, 8, 8, 1, 1)):
        assert L.kgdet_conv_apply_plan(*(args + (out.data_ptr(),))) == E_SHAPE
    assert L.kgdet_conv_grad_weight_plan(2, 128, 64, 8, 8, 9, out.data_ptr()) == 4          # C % 128 != 0: unsupported
    assert L.kgdet_conv_grad_weight_plan(2, 128, 128, 8, 8, 1, out.data_ptr()) == E_SHAPE    # a 1x1 problem has H = 1
    assert (out == 77).all()
    assert CANARY != 77
