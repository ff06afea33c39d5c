"""The fused serial / parallel head loss kernels -- csrc/serial_loss.hip: serial_init_select, serial_refine_iou,
serial_assign_finish, serial_loss_rows forward / backward, serial_loss_finish -- through the C ABI (kgdet_serial_loss_forward /
_backward with the ctypes structs of kgdet_amd/serial_loss.py) against the references of tests/serial_loss_refs.py.

The discrete decisions and the arithmetic are judged apart.  The two assignments and the best IoU are read back from the
workspace (the layout pinned in include/kgdet_hip.h):
  refine   EXACTLY assign_max_iou of the numpy float32 restatement of bbox_overlaps on centre + box * stride (the IoU is
           bit-equal: no margin);
  init     a correct assigner's within M = 8 * 2^-24 of every float64 distance (head_loss_refs.check_assignment), and the
           float64 reference's own answer where the margins decide (every generated case: asserted on the CPU in
           tests/test_serial_loss_refs.py) or every operation is exact (the pinned cases).
Losses and gradients are then compared with the float64 evaluation OF THE KERNEL'S OWN ASSIGNMENTS inside
serial_loss_refs.bars: 4 x the error of a float32 restatement, with a floor of the output's own last roundings.  Nothing is taken
from the kernel.  Outputs and workspace sit inside canaries and are pre-filled with NaN.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import head_loss_refs as H
from tests import serial_loss_refs as R

pytestmark = pytest.mark.gpu

CANARY = 12345.678
WORST = {}           # output family -> the worst error seen, as a fraction of its bar (printed by every case)


def _L():
    from kgdet_amd import _lib
    return _lib, _lib.lib()


class Guarded(object):
    """``n`` floats of NaN at 64 floats into a buffer of CANARY"""

    def __init__(self, n, lead=64, tail=64):
        self.n, self.lead = n, lead
        self.buf = torch.full((lead + n + tail,), CANARY, dtype=torch.float32, device='cuda')
        self.view().fill_(float('nan'))

    def view(self):
        return self.buf[self.lead:self.lead + self.n]

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lead

    def intact(self):
        return bool((self.buf[:self.lead] == CANARY).all()) and bool((self.buf[self.lead + self.n:] == CANARY).all())

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.view()).all())


class Call(object):
    """the device side of one case: ground truth, maps, descriptors, outputs inside canaries"""

    def __init__(self, case):
        from kgdet_amd import serial_loss as SL
        lib, L = _L()
        self.case = case
        dev = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
        self.keep = []
        t = SL.SerialTargets()
        t.B, t.L, t.num_classes, t.num_keypoints = case.B, case.L, case.C, case.K
        for l in range(case.L):
            t.H[l], t.W[l], t.stride[l] = case.shapes[l][0], case.shapes[l][1], case.strides[l]
        for b in range(case.B):
            bb, kp = dev(case.boxes[b]), dev(case.kps[b])
            lab = None if case.labels is None else dev(case.labels[b], np.int64)
            self.keep += [bb, kp, lab]
            t.num_gt[b] = len(case.boxes[b])
            t.gt_bboxes[b], t.gt_keypoints[b] = bb.data_ptr(), kp.data_ptr()
            t.gt_labels[b] = None if lab is None else lab.data_ptr()
            for l in range(case.L):
                t.valid_h[b][l], t.valid_w[b][l] = case.valid[b][l]
        c = SL.SerialLossCfg()
        for n in ('pos_num', 'scale', 'pos_iou_thr', 'neg_lo', 'neg_hi', 'min_pos_iou', 'pos_weight', 'point_base_scale', 'gamma',
                  'alpha'):
            setattr(c, n, getattr(case, n))
        for k in range(4):
            c.beta[k] = case.beta[k]
        for k in range(5):
            c.loss_weight[k] = case.loss_weight[k]
        self.t, self.c = t, c
        self.maps = [dev(case.maps[n][l]) for n in R.FAMILIES for l in range(case.L)]
        self.hm = SL._maps(self.maps, case.L)
        self.up = dev(np.asarray(case.upstream, np.float32))
        self.ws_bytes = L.kgdet_serial_loss_workspace_bytes(ctypes.byref(t), ctypes.byref(c))
        self.ws = Guarded((self.ws_bytes + 3) // 4)
        self.out = Guarded(5 * case.L + 2)
        self.grads = [Guarded(m.numel()) for m in self.maps]
        hg = SL.SerialMaps()
        for f, n in enumerate(R.FAMILIES):
            for l in range(case.L):
                getattr(hg, n)[l] = self.grads[f * case.L + l].ptr()
        self.hg = hg

    def forward(self, ws_bytes=None):
        lib, L = _L()
        return L.kgdet_serial_loss_forward(ctypes.byref(self.t), ctypes.byref(self.c), ctypes.byref(self.hm),
                                           ctypes.c_void_p(self.out.ptr()), ctypes.c_void_p(self.out.ptr() + 20 * self.case.L),
                                           ctypes.c_void_p(self.ws.ptr()), ctypes.c_size_t(self.ws_bytes if ws_bytes is None else ws_bytes),
                                           lib.current_stream())

    def backward(self, ws_bytes=None):
        lib, L = _L()
        return L.kgdet_serial_loss_backward(ctypes.byref(self.t), ctypes.byref(self.c), ctypes.byref(self.hm),
                                            ctypes.c_void_p(self.up.data_ptr()), ctypes.c_void_p(self.out.ptr() + 20 * self.case.L),
                                            ctypes.byref(self.hg), ctypes.c_void_p(self.ws.ptr()),
                                            ctypes.c_size_t(self.ws_bytes if ws_bytes is None else ws_bytes), lib.current_stream())

    def nothing_written(self):
        torch.cuda.synchronize()
        return self.out.untouched() and self.ws.untouched() and all(g.untouched() for g in self.grads)

    def assignments(self):
        """(assigned_init, assigned_refine, best_iou) [B, N]: the first three tables of the workspace, at bytes 0, T and 2 T with
        T = B * N * 4 rounded up to 256 (include/kgdet_hip.h)"""
        case = self.case
        n = case.B * case.N
        step = (n * 4 + 255) // 256 * 64                       # floats
        raw = self.ws.view()[:3 * step].cpu().numpy()
        ints = raw.view(np.int32)
        return (ints[:n].reshape(case.B, -1).astype(np.int64), ints[step:step + n].reshape(case.B, -1).astype(np.int64),
                raw[2 * step:2 * step + n].reshape(case.B, -1))


def _note(family, err, bar, tag):
    r = 0.0 if err == 0 else (float('inf') if bar == 0 else err / bar)
    WORST[family] = max(WORST.get(family, 0.0), r)
    print('%s: error %.3e, bar %.3e (%.3f of it); worst so far: %s' % (tag, err, bar, r, {k: round(v, 3) for k, v in WORST.items()}))
    return r


def _check_case(case, want=None):
    lib, L = _L()
    call = Call(case)
    lib.check(call.forward(), 'kgdet_serial_loss_forward')
    lib.check(call.backward(), 'kgdet_serial_loss_backward')
    torch.cuda.synchronize()
    out = call.out.view().cpu().numpy()
    first = [out.copy()] + [g.view().clone() for g in call.grads]
    ai, ar, best = call.assignments()
    nl = case.L

    # 1. refine: exactly the restated assigner; best IoU bit for bit
    for b in range(case.B):
        want_ar, want_best = R.refine_reference(case, b)
        assert (best[b].view(np.int32) == want_best.view(np.int32)).all(), 'image %d: best IoU differs' % b
        assert (ar[b] == want_ar).all(), 'image %d: not the reference refine assignment' % b
    # 2. init: a correct assigner's; the reference's own (margins beyond 64 M, or exact arithmetic)
    for b in range(case.B):
        D = R.init_distances(case, b)
        H.check_assignment(ai[b], D, case.pos_num)
        assert (ai[b] == R.init_reference(case, b)).all(), 'image %d: not the reference init assignment' % b
    for b, table in ((0, want or {}),):
        for i, v in table.get('init', {}).items():
            assert ai[b][i] == v
        for i, v in table.get('refine', {}).items():
            assert ar[b][i] == v
        for i, v in table.get('best', {}).items():
            assert float(best[b][i]) == v
        if 'init_count' in table:
            assert (ai[b] > 0).sum() == table['init_count']
        if 'refine_all' in table:
            assert (ar[b] == table['refine_all']).all()
        if 'refine_positives' in table:
            assert (ar[b] > 0).sum() == table['refine_positives']
    # 3. num_total of both stages from the assignments, exactly
    totals = R.num_totals(list(ai), list(ar))
    assert (out[5 * nl], out[5 * nl + 1]) == totals, (out[5 * nl:], totals)
    # 4. canaries, no NaN left
    assert call.out.intact() and call.ws.intact() and all(g.intact() for g in call.grads)
    assert np.isfinite(out).all()

    # 5. losses and gradients of the kernel's own assignments inside the bars; the exact-zero patterns
    ref = R.losses_and_grads(case, list(ai), list(ar))
    res = R.losses_and_grads(case, list(ai), list(ar), f32=True)
    loss_bar, grad_bar = R.bars(ref, res)
    worst = 0.0
    got_l = out[:5 * nl].reshape(5, nl)
    for k in range(5):
        for l in range(nl):
            worst = max(worst, _note('loss_' + R.kind_of(k), abs(float(got_l[k, l]) - ref[0][k, l]), loss_bar[k, l],
                                     '%s %s level %d' % (case.name, R.NAMES[k], l)))
    off = case.offsets
    for k in range(5):
        for l in range(nl):
            want_g = ref[2][(k, l)]
            got = call.grads[k * nl + l].view().cpu().numpy().reshape(want_g.shape)
            assert np.isfinite(got).all(), 'gradient map %s level %d holds a NaN or an infinity' % (R.FAMILIES[k], l)
            worst = max(worst, _note('grad_' + R.kind_of(k), float(np.abs(got - want_g).max()), grad_bar[(k, l)],
                                     '%s grad %s level %d' % (case.name, R.FAMILIES[k], l)))
            assert (got[want_g == 0] == 0).all(), 'map %s level %d: non-zero where the reference is exactly zero' % (R.FAMILIES[k], l)
            for b in range(case.B):
                inside = case.valid_mask(b)[off[l]:off[l + 1]]
                assert (got[b][:, ~inside] == 0).all(), 'a gradient outside the valid extent'
                if k > 0:
                    a = (ai if R.STAGE[k] == 0 else ar)[b][off[l]:off[l + 1]]
                    assert (got[b][:, a <= 0] == 0).all(), 'a regression gradient at a point that is no positive'
    assert worst <= 1.0, 'an output is %.3f of its bar away' % worst

    # 6. a second forward + backward: the same bits
    call.ws.view().fill_(float('nan'))
    lib.check(call.forward(), 'kgdet_serial_loss_forward')
    lib.check(call.backward(), 'kgdet_serial_loss_backward')
    torch.cuda.synchronize()
    assert (call.out.view().cpu().numpy().view(np.int32) == first[0].view(np.int32)).all()
    for k in range(5 * nl):
        assert torch.equal(call.grads[k].view().view(torch.int32), first[1 + k].view(torch.int32)), k
    return call, ai, ar


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_generated_case(name):
    """random inputs whose init margins all exceed 64 M (per case: tests/serial_loss_refs.py CASES says which edge it is there
    for): both assignments equal the references', and every item of the list above holds"""
    _check_case(R.make_case(name))
    torch.cuda.empty_cache()


@pytest.mark.parametrize('name', R.PINNED)
def test_pinned_exact_case(name):
    """hand-made cases of exact arithmetic: level expression exactly 3, clamped levels, the tie rules of both assigners, a
    disjoint gt claiming every point at IoU 0, IoUs exactly at 0.4 and 0.5, a tuple neg_iou_thr, no refine positive"""
    case, want = R.pinned(name)
    case.name = name
    call, ai, ar = _check_case(case, want)
    if name == 'no_refine_positive':
        assert float(call.out.view()[5 * case.L + 1]) == 1.0            # max(0, 1)
        for k in (2, 4):                                                   # no refine positive: zero regression losses
            assert (call.out.view()[k * case.L:(k + 1) * case.L] == 0).all()


# ============================================================================================ status codes
def _small():
    return R.make_case('small_b1')


@pytest.mark.parametrize('what', ['B17', 'gt0', 'gt65', 'levels9', 'strides_not_doubling', 'stride_not_power_of_two',
                                  'pos_num_beyond_valid', 'pos_num65', 'beta0', 'level_too_large'])
def test_rejected_arguments_write_nothing(what):
    lib, L = _L()
    call = Call(_small())
    if what == 'B17':
        call.t.B = 17
    elif what == 'gt0':
        call.t.num_gt[0] = 0
    elif what == 'gt65':
        call.t.num_gt[0] = 65
    elif what == 'levels9':
        call.t.L = 9
    elif what == 'strides_not_doubling':
        call.t.stride[2] = 64.0
    elif what == 'stride_not_power_of_two':
        call.t.stride[0] = 6.0
    elif what == 'pos_num_beyond_valid':
        call.c.pos_num = 2                       # the last level holds one point
    elif what == 'pos_num65':
        call.c.pos_num = 65
    elif what == 'beta0':
        call.c.beta[2] = 0.0
    elif what == 'level_too_large':
        call.t.H[0], call.t.W[0] = 182, 181
    assert call.forward() == lib.KGDET_E_SHAPE
    assert call.backward() == lib.KGDET_E_SHAPE
    assert call.nothing_written()


def test_short_workspace():
    lib, L = _L()
    call = Call(_small())
    assert call.forward(ws_bytes=call.ws_bytes - 1) == lib.KGDET_E_WORKSPACE
    assert call.forward(ws_bytes=0) == lib.KGDET_E_WORKSPACE
    assert call.backward(ws_bytes=call.ws_bytes - 1) == lib.KGDET_E_WORKSPACE
    assert call.nothing_written()
    assert call.forward() == lib.KGDET_OK
    torch.cuda.synchronize()
    assert call.ws.intact()                       # the size kgdet_serial_loss_workspace_bytes names is enough
