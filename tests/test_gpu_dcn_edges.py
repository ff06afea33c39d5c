"""GPU parity at the sampling edges: every deformable-convolution route against the float64 oracle on the inputs of
tests/dcn_edge_cases.py -- positions exactly on -1, on the lattice, on L-1 and L, a hair inside and outside of each, beyond the
int32 range, modulation masks with exact zeros -- on the smallest shapes that still reach each kernel.

The positions are exact in float32 (tests/test_dcn_edge_cases.py holds the inputs and the two oracles to each other on the CPU), so
EVERY element is compared: there is no "all but a few elements" allowance here.  Tolerances are those of tests/test_gpu_dcn.py for
the same kernels: forward 2e-5 of the output scale ('split', 'exact'), 1e-2 ('bf16'); every gradient 5e-5.

Which kernel serves which shape (csrc/dcn_api.hip; HW = H * W of the input map, kPlaneMaxHW = 1344):
  forward 'split' / 'bf16'   plane_ok (HW <= 1344): dcn_fwd_plane<2> / <1>;  else gather_ok: dcn_fwd_gather<2> / <1>
  forward 'exact'            always dcn_fwd_mfma (make_tap_pair, needs W >= 2)
  backward, default          HW <= 1344, plane_bwd_input_ok and plane_bwd_offset_ok: dcn_bwd_input_plane<2> (inverse records of
                             dcn_build_inverse_taps, overflow sums) + grad_offset on dcn_bwd_offset_pair (v1, Og % 32 == 0, K >= 3 and
                             the static schedule of plan_static_ranges: of these shapes only 2x32x6x7x32 -- with 16 channels the two
                             pixel tiles share one workgroup and run stream-K), dcn_bwd_offset_plane<2> (v1 otherwise) or
                             dcn_bwd_offset_plane_masked (v2), records of dcn_build_grad_taps;
                             grad_weight on dcn_bwd_weight_os<2> (all tiles in one round) or dcn_bwd_weight_plane<2> (stream-K option);
                             HW > 1344: dcn_backward_large.hip per channel run + dcn_bwd_weight_gather<2>
  backward, 'exact'          HW <= 1088 (plan_bwd_lds): dcn_bwd_build_index + dcn_bwd_input_gather (dcn_backward_gather.hip);
                             larger: dcn_backward_large.hip; grad_weight on dcn_bwd_weight_mfma (f32)
Narrow, numerous weight groups (8 ... 32 groups of 1 ... 32 channels, what a ResNeXt block's dcn['groups'] reaches) take other
rows of this table -- no plane backward kernel at all (plane_bwd_offset_ok), dcn_bwd_input_gather in BOTH arithmetics up to 1088
pixels, the zero-padded large-map route from 1089 pixels on, one dcn_bwd_weight_mfma per group beyond 8 channel runs --: the table
and the tests are in tests/test_gpu_dcn_groups.py.
"""
import functools

import numpy as np
import pytest
import torch

import oracle
from tests import dcn_edge_cases as E

pytestmark = pytest.mark.gpu

SEED = 7
PRECISIONS = [('split', 2e-5), ('exact', 2e-5), ('bf16', 1e-2)]
GRAD_TOL = 5e-5
GRADS_V1 = ('grad_input', 'grad_offset', 'grad_weight')
GRADS_V2 = GRADS_V1 + ('grad_mask', 'grad_bias')


def _require_gpu():
    assert torch.cuda.is_available(), 'GPU tests need a GPU (no fallback)'


@functools.lru_cache(maxsize=None)
def _ref(case, kind, v2):
    """float64 oracle of (case, offset kind, v1 / v2): computed once, shared by the tests, read-only"""
    return E.reference(case, kind, v2, SEED)


def _close(what, actual, desired, tol):
    """every element within `tol` of the oracle's scale; prints the figure before it asserts"""
    actual = actual.detach().cpu().numpy() if torch.is_tensor(actual) else actual
    assert actual.shape == desired.shape, (what, actual.shape, desired.shape)
    assert np.isfinite(actual).all(), '%s: non-finite values' % what
    scale = max(float(np.abs(desired).max()), 1e-6)
    err = float(np.abs(actual.astype(np.float64) - desired).max()) / scale
    print('EDGE-ERR %s err %.3e tol %.1e frac %.3f' % (what, err, tol, err / tol))
    assert err < tol, '%s: max error %.3e of the scale (tol %.1e)' % (what, err, tol)


def _cuda(a, grad=False):
    t = torch.from_numpy(np.array(a)).cuda()
    return t.requires_grad_() if grad else t


def _forward(r, case, v2, prec):
    from kgdet_amd import dcn
    N, C, H, W, O, k, s, p, d, g, dg = case
    with torch.no_grad(), dcn.forward_precision(prec):
        if v2:
            return dcn.modulated_deform_conv(_cuda(r['x']), _cuda(r['off']), _cuda(r['mask']), _cuda(r['w']), _cuda(r['bias']),
                                             s, p, d, g, dg)
        return dcn.deform_conv(_cuda(r['x']), _cuda(r['off']), _cuda(r['w']), s, p, d, g, dg)


def _autograd(r, case, v2):
    """forward + backward through the public functions: dict(y, grad_input, grad_offset, grad_weight[, grad_mask, grad_bias])"""
    from kgdet_amd import dcn
    N, C, H, W, O, k, s, p, d, g, dg = case
    tx, to, tw = (_cuda(r[n], True) for n in ('x', 'off', 'w'))
    if v2:
        tm, tb = _cuda(r['mask'], True), _cuda(r['bias'], True)
        y = dcn.modulated_deform_conv(tx, to, tm, tw, tb, s, p, d, g, dg)
    else:
        y = dcn.deform_conv(tx, to, tw, s, p, d, g, dg)
    y.backward(_cuda(r['go']))
    out = dict(y=y.detach(), grad_input=tx.grad, grad_offset=to.grad, grad_weight=tw.grad)
    if v2:
        out.update(grad_mask=tm.grad, grad_bias=tb.grad)
    return out


def _check_grads(tag, got, r, v2):
    for name in (GRADS_V2 if v2 else GRADS_V1):
        _close('%s %s' % (tag, name), got[name], r[name], GRAD_TOL)


def _poison_allocator():
    """fill the caching allocator's free blocks, small pool and large pool, with NaN: whatever a kernel leaves unwritten shows"""
    junk = [torch.full((128 * 1024,), float('nan'), device='cuda') for _ in range(32)]
    junk += [torch.full((8 * 1024 * 1024,), float('nan'), device='cuda') for _ in range(4)]
    del junk


# ---------------------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize('kind', ['edge', 'lattice'])
@pytest.mark.parametrize('case', E.CASES, ids=E.case_id)
def test_forward_all_precisions(case, kind):
    """v1 and v2 (edge mask, bias) under 'split', 'exact', 'bf16'.  Maps of at most 1344 pixels: dcn_fwd_plane<2> / dcn_fwd_plane<1>
    (plane_ok) and, for 'exact', dcn_fwd_mfma with make_tap_pair -- W == 2 puts x0 == -1 and x0 == W-1 on the one column pair,
    H == 1 leaves the high row dead everywhere.  38 x 36 (1368 pixels): dcn_fwd_gather (gather_ok) on corners gathered from the
    pixel-major copy of x.  `lattice`: the zero offsets init_offset() leaves."""
    _require_gpu()
    for v2 in (False, True):
        r = _ref(case, kind, v2)
        for prec, tol in PRECISIONS:
            y = _forward(r, case, v2, prec)
            _close('forward %s %s %s %s' % (E.case_id(case), kind, 'v2' if v2 else 'v1', prec), y, r['y'], tol)


# ------------------------------------------------------------------------------------------------------- 2. autograd backward
@pytest.mark.parametrize('kind', ['edge', 'lattice'])
@pytest.mark.parametrize('case', E.CASES, ids=E.case_id)
def test_backward_default_arithmetic(case, kind):
    """Autograd backward, v1 and v2, default (split-operand) arithmetic, twice with identical bits.  Maps of at most 1344 pixels
    (plane_bwd_input_ok, plane_bwd_offset_ok): grad_input on dcn_bwd_input_plane<2> from the inverse records -- the short palette on
    small maps sends dozens of contributions into every border cell, through the more-than-8-entry overflow records --, grad_offset
    on the tap-pair kernel (v1, 2x32x6x7x32), dcn_bwd_offset_plane<2> (v1, the others) or dcn_bwd_offset_plane_masked (v2, where a
    mask of exactly 0 must not kill grad_mask), grad_weight on the plane kernel.  38 x 36: dcn_backward_large.hip (inverse index per
    channel run) and dcn_bwd_weight_gather<2>."""
    _require_gpu()
    for v2 in (False, True):
        r = _ref(case, kind, v2)
        a, b = _autograd(r, case, v2), _autograd(r, case, v2)
        tag = 'backward %s %s %s' % (E.case_id(case), kind, 'v2' if v2 else 'v1')
        _close(tag + ' y', a['y'], r['y'], 2e-5)
        _check_grads(tag, a, r, v2)
        for name in a:
            assert torch.equal(a[name], b[name]), '%s %s differs between two runs' % (tag, name)


# ------------------------------------------------------------------------------------------------ 3. direct plane entry points
def _plane_map(case):
    return case[2] * case[3] <= 1344


GRAD_INPUT_CASES = [c for c in E.CASES if _plane_map(c)]
GRAD_OFFSET_CASES = [c for c in E.CASES if _plane_map(c) and (c[1] // c[9]) % (c[1] // c[10]) == 0 and c[4] // c[9] <= 256]
GRAD_WEIGHT_CASES = [c for c in E.CASES if _plane_map(c)]
assert GRAD_INPUT_CASES == GRAD_OFFSET_CASES == GRAD_WEIGHT_CASES == E.SMALL_CASES


@pytest.mark.parametrize('case', E.SMALL_CASES, ids=E.case_id)
def test_plane_entry_points_directly(case):
    """dcn.grad_input_plane (v1 and masked), dcn.grad_offset_plane and dcn.grad_weights_grouped decline instead of falling back, so a
    pass means the plane kernel computed the result: dcn_bwd_input_plane<2>; dcn_bwd_offset_pair for 2x32x6x7x32 and
    dcn_bwd_offset_plane<2> otherwise (offset_pair_ok); dcn_bwd_weight_os<2>, and dcn_bwd_weight_plane<2> under the stream-K option."""
    _require_gpu()
    from kgdet_amd import _lib, dcn
    N, C, H, W, O, k, s, p, d, g, dg = case
    r = _ref(case, 'edge', False)
    tx, to, tw, tg = (_cuda(r[n]) for n in ('x', 'off', 'w', 'go'))
    shape = dcn._shape(tx, tw, (s, s), (p, p), (d, d), g, dg)
    tag = 'plane %s' % E.case_id(case)
    gi = dcn.grad_input_plane(tx.shape, to, None, tw, tg, shape)
    assert torch.equal(gi, dcn.grad_input_plane(tx.shape, to, None, tw, tg, shape))
    _close(tag + ' grad_input', gi, r['grad_input'], GRAD_TOL)
    r2 = _ref(case, 'edge', True)        # (the same x, offsets, weight and grad_out, plus the edge mask)
    gim = dcn.grad_input_plane(tx.shape, to, _cuda(r2['mask']), tw, tg, shape)
    _close(tag + ' grad_input masked', gim, r2['grad_input'], GRAD_TOL)
    go = dcn.grad_offset_plane(tx, to, tw, tg, shape)
    assert torch.equal(go, dcn.grad_offset_plane(tx, to, tw, tg, shape))
    _close(tag + ' grad_offset', go, r['grad_offset'], GRAD_TOL)
    gw = dcn.grad_weights_grouped([tx], [to], [tg], [tw], [shape])
    assert gw is not None, 'the plane grad_weight kernel declined'
    _close(tag + ' grad_weight', gw[0], r['grad_weight'], GRAD_TOL)
    _lib.check(_lib.lib().kgdet_set_option(2, 1), 'kgdet_set_option')
    try:
        gws = dcn.grad_weights_grouped([tx], [to], [tg], [tw], [shape])
    finally:
        _lib.check(_lib.lib().kgdet_set_option(2, 0), 'kgdet_set_option')
    assert gws is not None, 'the stream-K grad_weight kernel declined'
    _close(tag + ' grad_weight stream-K', gws[0], r['grad_weight'], GRAD_TOL)


# ------------------------------------------------------------------------------------------------------ 4. exact arithmetic
@pytest.mark.parametrize('case', E.CASES, ids=E.case_id)
def test_backward_exact_arithmetic(case):
    """The same backward under dcn.arithmetic('exact'), v1 and v2.  H * W <= 1088 (plan_bwd_lds): dcn_bwd_build_index +
    dcn_bwd_input_gather of dcn_backward_gather.hip, grad_weight on the f32 kernel dcn_bwd_weight_mfma; 38 x 36:
    dcn_backward_large.hip, v1 and v2."""
    _require_gpu()
    from kgdet_amd import dcn
    for v2 in (False, True):
        r = _ref(case, 'edge', v2)
        with dcn.arithmetic('exact'):
            a = _autograd(r, case, v2)
        tag = 'exact %s %s' % (E.case_id(case), 'v2' if v2 else 'v1')
        _close(tag + ' y', a['y'], r['y'], 2e-5)
        _check_grads(tag, a, r, v2)


# ------------------------------------------------------------------------------------------------- 5. grouped head-stage launch
CAT_KS = (3, 5, 7)


def _cat_case(k):
    return (2, 16, 6, 7, 16, k, 1, k // 2, 1, 1, 1)


@functools.lru_cache(maxsize=None)
def _cat_inputs(outside_k):
    rng = np.random.default_rng(SEED)
    xs = [rng.normal(size=(2, 16, 6, 7)).astype(np.float32) for _ in range(2)]
    offs = [E.all_outside(_cat_case(k)) if k == outside_k else E.edge_offsets(_cat_case(k), SEED + k) for k in CAT_KS]
    ws = [[(rng.normal(size=(16, 16, k, k)) * 0.05).astype(np.float32) for k in CAT_KS] for _ in xs]
    gos = [rng.normal(size=(2, 48, 6, 7)).astype(np.float32) for _ in xs]
    f64 = lambda a: a.astype(np.float64)
    ys = [np.concatenate([oracle.deform_conv_forward(f64(xs[i]), f64(offs[j]), f64(ws[i][j]), 1, k // 2, 1)
                          for j, k in enumerate(CAT_KS)], 1) for i in range(2)]
    return xs, offs, ws, gos, ys


@pytest.mark.parametrize('outside_k', [None, 5], ids=['edge', 'outside5x5'])
@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
def test_grouped_head_stage_launch(relu, outside_k, monkeypatch):
    """dcn.deform_conv_cat_multi: two maps [2, 16, 6, 7] x 3x3 / 5x5 / 7x7 (16 output channels each) as one grouped launch each way
    -- dcn_fwd_plane<2>, then dcn_bwd_input_plane<2> with the grouped grad_offset launch, and the grouped grad_weight launch.  The
    autograd function falls back to one call per problem when a grouped entry point declines, so the two backward entry points
    are watched: the grouped grad_weight call and the last grouped grad_input / grad_offset call must return KGDET_OK, i.e. the
    grouped kernels computed every gradient checked here.  The offsets are shared by the two maps.  The variant that lets the
    fix-up kernels sum the problems sharing an output needs the static schedule (plan_static_ranges), which six problems of 9 / 25
    / 49 one-chunk stages do not get (ranges too uneven): on this shape that first call declines before it launches anything and the
    grouped launch runs once more with one output per problem, summed per map / per offset tensor by the caller.  With ReLU the forward is checked first and the
    reference gradients take the ReLU mask of the KERNEL's output (an element within rounding of zero may flip in float64).
    `outside5x5`: the 5x5 offsets are all +1e4 (the call shares one offset tensor per kernel size between the maps, so both maps'
    5x5 problems are dead): their windows of the outputs, grad_offset and both grad_weights are exactly 0 while the 3x3 and 7x7
    problems of the same launches still agree with the oracle."""
    _require_gpu()
    from kgdet_amd import _lib, dcn
    xs, offs, ws, gos, ys = _cat_inputs(outside_k)
    txs, tos = [_cuda(x, True) for x in xs], [_cuda(o, True) for o in offs]
    tws = [[_cuda(w, True) for w in wl] for wl in ws]
    outs = dcn.deform_conv_cat_multi(txs, tos, tws, [k // 2 for k in CAT_KS], relu=relu)
    L, status = _lib.lib(), {}
    for entry in ('kgdet_deform_conv_backward_input_grouped', 'kgdet_deform_conv_grad_weight_grouped'):
        def watched(*args, _entry=entry, _call=getattr(L, entry)):
            rc = _call(*args)
            status.setdefault(_entry, []).append(rc)
            return rc
        monkeypatch.setattr(L, entry, watched)
    tag = 'cat_multi %s %s' % ('relu' if relu else 'linear', outside_k)
    got_y = [o.detach().cpu().numpy() for o in outs]
    for i in range(2):
        _close('%s y[%d]' % (tag, i), got_y[i], np.maximum(ys[i], 0.0) if relu else ys[i], 2e-5)
    torch.autograd.backward(outs, [_cuda(g) for g in gos])
    io, gw = status.get('kgdet_deform_conv_backward_input_grouped', []), status.get('kgdet_deform_conv_grad_weight_grouped', [])
    assert gw == [_lib.KGDET_OK], 'the grouped grad_weight launch declined: %r' % status
    assert io and io[-1] == _lib.KGDET_OK and set(io[:-1]) <= {_lib.KGDET_E_UNSUPPORTED}, \
        'the grouped grad_input / grad_offset launch declined: %r' % status
    f64 = lambda a: a.astype(np.float64)
    ref_x = [np.zeros(xs[0].shape) for _ in xs]
    ref_o = [np.zeros(o.shape) for o in offs]
    for i in range(2):
        go = f64(gos[i]) * (got_y[i] > 0) if relu else f64(gos[i])
        for j, k in enumerate(CAT_KS):
            rb = oracle.deform_conv_backward(f64(xs[i]), f64(offs[j]), f64(ws[i][j]), go[:, 16 * j:16 * (j + 1)], 1, k // 2, 1)
            ref_x[i] += rb['grad_input']
            ref_o[j] += rb['grad_offset']
            if k == outside_k:
                assert not rb['grad_weight'].any() and not rb['grad_offset'].any() and not rb['grad_input'].any()
                assert not tws[i][j].grad.cpu().numpy().any(), 'grad_weight of a dead problem must be exactly 0'
            else:
                _close('%s grad_weight[%d][%d]' % (tag, i, k), tws[i][j].grad, rb['grad_weight'], GRAD_TOL)
    for i in range(2):
        _close('%s grad_input[%d]' % (tag, i), txs[i].grad, ref_x[i], GRAD_TOL)
    for j, k in enumerate(CAT_KS):
        if k == outside_k:
            assert not tos[j].grad.cpu().numpy().any(), 'grad_offset of a dead problem must be exactly 0'
            for i in range(2):
                assert not got_y[i][:, 16 * j:16 * (j + 1)].any(), 'the output window of a dead problem must be exactly 0'
        else:
            _close('%s grad_offset[%d]' % (tag, k), tos[j].grad, ref_o[j], GRAD_TOL)


# ---------------------------------------------------------------------------------------------------------- 6. nothing alive
def _exactly(what, actual, desired):
    actual = actual.detach().cpu().numpy()
    assert np.isfinite(actual).all(), '%s: non-finite values (an element was not written)' % what
    assert np.array_equal(actual.astype(np.float64), desired), '%s: not exactly the oracle\'s values' % what


@pytest.mark.parametrize('v2', [False, True], ids=['v1', 'v2'])
@pytest.mark.parametrize('case', [E.CASES[1], E.CASES[8]], ids=E.case_id)
def test_all_outside_every_element_is_written(case, v2):
    """Every offset +1e4, through the single-call routes of the tests above (forward in three precisions, backward in the default and
    in the exact arithmetic), on the 6 x 7 plane shape and on 38 x 36, with the allocator's free blocks filled with NaN before each
    call: y is exactly 0 (v2: exactly the bias), every gradient exactly 0 -- written by the kernels, not left over.  The autograd routes
    hand the kernels a zeroed grad_input (dcn._backward), so there the poison shows unwritten elements of y, grad_offset, grad_mask
    and grad_weight only; for grad_input the 6 x 7 shape also calls dcn.grad_input_plane, which allocates uninitialised memory.
    grad_bias, the one sum that does not depend on the sampling (a float32 sum of grad_out cannot match a float64 sum bit for bit),
    is held to the gradient tolerance."""
    _require_gpu()
    from kgdet_amd import dcn
    r = _ref(case, 'outside', v2)
    assert not r['grad_input'].any() and not r['grad_offset'].any() and not r['grad_weight'].any()
    tag = 'outside %s %s' % (E.case_id(case), 'v2' if v2 else 'v1')
    for prec, _ in PRECISIONS:
        _poison_allocator()
        _exactly('%s y %s' % (tag, prec), _forward(r, case, v2, prec), r['y'])
    for mode in ('split', 'exact'):
        _poison_allocator()
        with dcn.arithmetic(mode):
            a = _autograd(r, case, v2)
        _exactly('%s y (%s)' % (tag, mode), a['y'], r['y'])
        for name in GRADS_V1 + (('grad_mask',) if v2 else ()):
            _exactly('%s %s (%s)' % (tag, name, mode), a[name], r[name])
        if v2:
            _close('%s grad_bias (%s)' % (tag, mode), a['grad_bias'], r['grad_bias'], GRAD_TOL)
    if _plane_map(case):
        N, C, H, W, O, k, s, p, d, g, dg = case
        tx, to, tw, tg = (_cuda(r[n]) for n in ('x', 'off', 'w', 'go'))
        tm = _cuda(r['mask']) if v2 else None
        shape = dcn._shape(tx, tw, (s, s), (p, p), (d, d), g, dg)
        _poison_allocator()
        _exactly('%s grad_input_plane' % tag, dcn.grad_input_plane(tx.shape, to, tm, tw, tg, shape), r['grad_input'])
