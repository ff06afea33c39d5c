"""GPU parity of csrc/psroi.hip at its edges: every case of tests/psroi_edge_cases.py through deform_roi_pooling, forward and
backward, against the float64 oracle and the serial float32 oracle (tests/test_psroi_edge_cases.py holds the cases and the two
oracles to each other on the CPU).

Per case: `count` exactly; `out`, `grad_data`, `grad_trans` finite everywhere and within the case's bar of the float64 oracle, ALL
elements, relative to the oracle's scale; `out` and `grad_data` bit-equal to the serial float32 oracle (same products, same
order, no contraction -- the forward adds in the reference's own sample order, so it is held to bits as well); a second run through
the C ABI into NaN-filled outputs after poisoning the allocator gives the same bits again.  The bar of a quantity is 4 x the float32
oracle's own distance from the float64 oracle on that case, never below 8 x 2^-24 (psroi_edge_cases.bar): the kernels form the
float32 oracle's products and add them in another order, the factor covers order, not wrong terms.

Which kernel serves which case (kgdet_deform_psroi_forward / _backward):
  forward       psroi_to_cell_major (64-pixel x 64-channel tiles) + psroi_gather<0>, block = (RoI, class, 64-channel chunk)
  grad_trans    psroi_gather<1>, block = (RoI, class), 64 channels per round, bins folded into offset cells
  grad_data     default: psroi_prepare, psroi_quotient_t, psroi_list_alloc / _fill / _sort / _sort_long, then
                psroi_grad_data_lists<4> (channels per class % 4 == 0) or <1>, psroi_zero_tail for C > out_dim * G^2;
                KGDET_PSROI_GRAD_DATA=tiles (read once per process: a child process, tests/psroi_tiles_child.py):
                psroi_grad_data<4> / <13> / <32> by P*P*S*S <= 256 / <= 832 / more, list_cap segments of 4096 RoIs

Largest fraction err / bar per quantity over all cases (MI355X; each comparison prints a PSROI-ERR line):
  out         0.250 (rec1024)   -- bit-equal to the float32 oracle in every case, so this is the oracle's own fraction
  grad_data   0.250 (base), both routes -- likewise bit-equal
  grad_trans  0.250 (pp81, g7s1, rec1936, map9x15, noroi), 0.236 (prod), both routes with the same figures: where the largest
              error sits, the kernel's sum rounds as the serial float32 sum does; 0.013 (ch264) at the other end
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import psroi_edge_cases as E
from tests import psroi_tiles_child as K

pytestmark = pytest.mark.gpu


def _require_gpu():
    assert torch.cuda.is_available(), 'GPU tests need a GPU (no fallback)'


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else t


def _within_bar(case, what, got, r, name):
    """every element finite and within the case's bar of the float64 oracle; prints the figure before it asserts"""
    got = _np(got)
    ref64, ref32 = r[name], r[name + '32']
    assert got.shape == ref64.shape and got.dtype == np.float32, (what, got.shape, got.dtype)
    assert np.isfinite(got).all(), '%s %s %s: non-finite values (an element was not written)' % (case.name, what, name)
    scale, bar = E.bar(ref32, ref64)
    err = float(np.abs(got.astype(np.float64) - ref64).max()) / scale
    print('PSROI-ERR %s %s %s err %.3e bar %.3e frac %.3f' % (case.name, what, name, err, bar, err / bar))
    assert err < bar, '%s %s %s: max error %.3e of the scale, bar %.3e' % (case.name, what, name, err, bar)


def _bit_equal(case, what, got, want):
    got, want = _np(got), _np(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    same = got.view(np.uint32) == want.view(np.uint32)
    # +0 against -0 is the one difference in bits that is no difference in value; it does not occur, so it is not excused
    assert same.all(), '%s %s: %d of %d elements differ in bits, first at %s' % (
        case.name, what, int((~same).sum()), same.size, tuple(int(i[0]) for i in np.nonzero(~same)))


def _check_gradients(case, what, r, grad_data, grad_trans):
    _within_bar(case, what, grad_data, r, 'grad_data')
    _bit_equal(case, what + ' grad_data against the serial float32 oracle', grad_data, r['grad_data32'])
    dead = E.empty_group_channels(case)
    assert not _np(grad_data)[:, dead].any(), '%s %s: channels that own no bin must have gradient exactly 0' % (case.name, what)
    if not case.no_trans:
        _within_bar(case, what, grad_trans, r, 'grad_trans')
        ok = E.valid_rows(case, r['rois'])
        assert not _np(grad_trans)[~ok].any(), '%s %s: RoIs outside the batch must have grad_trans exactly 0' % (case.name, what)
        assert not _np(grad_trans)[:, :, E.empty_offset_cells(case)].any(), \
            '%s %s: offset cells that own no bin must have grad_trans exactly 0' % (case.name, what)
        if case.trans_std == 0.0:
            assert not _np(grad_trans).any()


# ------------------------------------------------------------------------------------------------- 1. every case, default route
@pytest.mark.parametrize('case', E.CASES, ids=E.case_id)
def test_forward_and_backward_against_both_oracles(case):
    _require_gpu()
    assert 'KGDET_PSROI_GRAD_DATA' not in os.environ
    r = E.reference(case)
    K.poison_allocator()
    a = K.autograd(case, r)
    assert np.array_equal(_np(a['count']), r['count32']) and np.array_equal(_np(a['count']).astype(np.float64), r['count'])
    _within_bar(case, 'lists', a['out'], r, 'out')
    _bit_equal(case, 'out against the float32 oracle', a['out'], r['out32'])
    _check_gradients(case, 'lists', r, a['grad_data'], a['grad_trans'])
    # second run: the C ABI into NaN-filled outputs, the allocator's free blocks full of NaN
    K.poison_allocator()
    out2, count2 = K.forward_abi(case, r)
    _bit_equal(case, 'out, second run', out2, a['out'])
    _bit_equal(case, 'count, second run', count2, a['count'])
    K.poison_allocator()
    gd2, gt2 = K.backward_abi(case, r, count2)
    _bit_equal(case, 'grad_data, second run', gd2, a['grad_data'])
    if not case.no_trans:
        assert np.isfinite(_np(gt2)).all()
        _bit_equal(case, 'grad_trans, second run', gt2, a['grad_trans'])


# ------------------------------------------------------------------------------------------------------------- 2. tile route
def test_tile_gather_route_in_a_fresh_process(tmp_path):
    """KGDET_PSROI_GRAD_DATA=tiles is read once per process: ONE child runs every case's backward on psroi_grad_data<4> / <13> /
    <32>.  Its workspace is smaller than this process's for the same shape -- the list arrays are absent on the tile route -- which
    is the proof that the route was taken; its gradients are held to the assertions of the list route."""
    _require_gpu()
    assert 'KGDET_PSROI_GRAD_DATA' not in os.environ
    path = str(tmp_path / 'tiles.npz')
    env = dict(os.environ, KGDET_PSROI_GRAD_DATA='tiles')
    res = subprocess.run([sys.executable, K.__file__, path], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert res.returncode == 0, 'the tile-route child failed (status %d):\n%s' % (
        res.returncode, res.stderr.decode('utf-8', 'replace')[-3000:])
    got = np.load(path)
    for case in E.CASES:
        r = E.reference(case)
        mine, theirs = K.backward_workspace_bytes(case), int(got[case.name + '/workspace'])
        assert 0 < theirs < mine, '%s: workspace %d in the child, %d here' % (case.name, theirs, mine)
        gd = got[case.name + '/grad_data']
        gt = None if case.no_trans else got[case.name + '/grad_trans']
        _check_gradients(case, 'tiles', r, gd, gt)
        _bit_equal(case, 'tiles grad_data, second run', got[case.name + '/grad_data_abi'], gd)
        if not case.no_trans:
            _bit_equal(case, 'tiles grad_trans, second run', got[case.name + '/grad_trans_abi'], gt)


# --------------------------------------------------------------------------------------------------------------- 3. refusals
_BASE = E.BY_NAME['base']
REFUSALS = {
    'P17': _BASE._replace(pooled_size=17, part_size=17, sample_per_part=1),
    'P16_S3': _BASE._replace(pooled_size=16, part_size=16, sample_per_part=3),
    'G17': _BASE._replace(group_size=17, C=8 * 17 * 17),
    'C_too_small': _BASE._replace(group_size=2, C=31),
    'trans_std_1.5': _BASE._replace(trans_std=1.5),
    'out_dim_mod_classes': _BASE._replace(num_classes=3),
    'map_side_32768': _BASE._replace(B=1, C=8, H=1, W=32768),
}
assert REFUSALS['P16_S3'].pooled_size ** 2 * 9 == 2304


def _random_call(case):
    """device tensors of the right shapes for `case` (which need not be inside the envelope) and NaN-filled outputs"""
    c = case
    rng = np.random.default_rng(3)
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()
    t = dict(data=f(c.B, c.C, c.H, c.W), grad_out=f(c.R, c.out_dim, c.pooled_size, c.pooled_size),
             offset=f(c.R, 2 * c.num_classes, c.part_size, c.part_size) * 0.1)
    rois = np.tile(np.array([[0, 8, 8, 71, 55]], np.float32), (c.R, 1))
    t['rois'] = torch.from_numpy(rois).cuda()
    nan = lambda like: torch.full_like(like, float('nan'))
    t.update(out=nan(t['grad_out']), count=nan(t['grad_out']), grad_data=nan(t['data']), grad_trans=nan(t['offset']))
    return t


def _call_both(case, t, fwd_bytes=None, bwd_bytes=None):
    """(status of kgdet_deform_psroi_forward, status of kgdet_deform_psroi_backward) on the tensors of _random_call; the workspace
    is the one the library asks for unless a size is given"""
    from kgdet_amd import _lib
    L, shape = _lib.lib(), K.shape_of(case)
    need_f = int(L.kgdet_deform_psroi_forward_workspace_bytes(ctypes.byref(shape)))
    need_b = int(L.kgdet_deform_psroi_backward_workspace_bytes(ctypes.byref(shape)))
    ws = torch.empty(max(need_f, need_b, 1), dtype=torch.uint8, device='cuda')
    cnt = torch.ones_like(t['grad_out'])
    rc_f = L.kgdet_deform_psroi_forward(
        ctypes.byref(shape), _lib.ptr(t['data']), _lib.ptr(t['rois']), _lib.ptr(t['offset']), _lib.ptr(t['out']),
        _lib.ptr(t['count']), _lib.ptr(ws), ctypes.c_size_t(need_f if fwd_bytes is None else fwd_bytes), _lib.current_stream())
    rc_b = L.kgdet_deform_psroi_backward(
        ctypes.byref(shape), _lib.ptr(t['grad_out']), _lib.ptr(cnt), _lib.ptr(t['data']), _lib.ptr(t['rois']),
        _lib.ptr(t['offset']), _lib.ptr(t['grad_data']), _lib.ptr(t['grad_trans']), _lib.ptr(ws),
        ctypes.c_size_t(need_b if bwd_bytes is None else bwd_bytes), _lib.current_stream())
    torch.cuda.synchronize()
    return rc_f, rc_b, need_f, need_b


def _untouched(t):
    return all(bool(torch.isnan(t[n]).all()) for n in ('out', 'count', 'grad_data', 'grad_trans'))


@pytest.mark.parametrize('name', sorted(REFUSALS))
def test_shapes_outside_the_envelope_are_refused(name):
    """psroi_check: KGDET_E_SHAPE from both entry points, nothing written, and an exception through the Python op"""
    _require_gpu()
    from kgdet_amd import _lib
    from kgdet_amd.deform_pool import deform_roi_pooling
    case = REFUSALS[name]
    t = _random_call(case)
    rc_f, rc_b, _, _ = _call_both(case, t)
    assert (rc_f, rc_b) == (_lib.KGDET_E_SHAPE, _lib.KGDET_E_SHAPE), (name, rc_f, rc_b)
    assert _untouched(t), '%s: a refused call wrote to its outputs' % name
    with pytest.raises((RuntimeError, AssertionError)):
        deform_roi_pooling(t['data'], t['rois'], t['offset'], *K.op_args(case))
    rc_f, rc_b, _, _ = _call_both(_BASE, _random_call(_BASE))       # (the same harness on the shape they were derived from)
    assert (rc_f, rc_b) == (_lib.KGDET_OK, _lib.KGDET_OK)


def test_a_workspace_one_byte_short_is_refused():
    _require_gpu()
    from kgdet_amd import _lib
    t = _random_call(_BASE)
    _, _, need_f, need_b = _call_both(_BASE, _random_call(_BASE))
    rc_f, rc_b, _, _ = _call_both(_BASE, t, fwd_bytes=need_f - 1, bwd_bytes=need_b - 1)
    assert (rc_f, rc_b) == (_lib.KGDET_E_WORKSPACE, _lib.KGDET_E_WORKSPACE)
    assert _untouched(t), 'a refused call wrote to its outputs'


@pytest.mark.parametrize('no_trans', [False, True], ids=['trans', 'no_trans'])
def test_no_rois_gives_an_empty_output_and_a_zero_gradient(no_trans):
    _require_gpu()
    from kgdet_amd.deform_pool import deform_roi_pooling
    case = _BASE._replace(R=0, no_trans=no_trans)
    t = _random_call(case)
    td, to = t['data'].requires_grad_(), t['offset'].requires_grad_()
    assert t['rois'].shape == (0, 5) and to.shape == (0, 4, 4, 4)
    K.poison_allocator()
    out = deform_roi_pooling(td, t['rois'], td.new_empty(0) if no_trans else to, *K.op_args(case))
    assert out.shape == (0, case.out_dim, case.pooled_size, case.pooled_size)
    out.backward(torch.empty_like(out))
    torch.cuda.synchronize()
    assert td.grad.shape == td.shape and not _np(td.grad).any() and np.isfinite(_np(td.grad)).all()
    if not no_trans:
        assert to.grad is not None and to.grad.shape == to.shape
