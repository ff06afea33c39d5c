"""The fused head-loss kernels -- csrc/head_loss.hip: head_assign_select, head_loss_rows forward / backward, head_loss_finish --
through the C ABI (kgdet_head_loss_forward / _backward with the ctypes structs of kgdet_amd/head_loss.py) against the float64
reference of tests/head_loss_refs.py, over the envelope include/kgdet_hip.h promises: B <= 16, 1 .. 64 gts per image,
H * W <= 4096, any pos_num, per-image valid extents.

The discrete decisions and the arithmetic are judged apart.  The kernel's selections are read back from the workspace
(dsel[b][g][i], row stride 64, +inf = not selected: the layout pinned in the header) and must satisfy what any correct assigner
satisfies (head_loss_refs.check_assignment); where the reference alone decides ('decided' and 'exact' regimes, conditions asserted
on the CPU in tests/test_head_loss_refs.py) they must equal it.  Losses and gradients are then compared with the float64
evaluation OF THE KERNEL'S OWN ASSIGNMENT, so a failure there is arithmetic and never a tie.

Bars (head_loss_refs.bars): 4 x the error of a float32 restatement -- one rounding per operation, serial sums -- against float64
on the same inputs, as a fraction of the output's scale, with a floor of the output's own last roundings.  Nothing is taken from
the kernel.  Outputs sit inside canaries and are pre-filled with NaN, and so is the workspace.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import head_loss_refs as R

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
        from kgdet_amd import head_loss as HL
        lib, L = _L()
        self.case = case
        dev = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
        self.keep = []
        t = HL.HeadTargets()
        t.B, t.H, t.W, t.num_classes, t.num_keypoints, t.stride = case.B, case.H, case.W, case.C, case.K, case.stride
        for b in range(case.B):
            bb, kp = dev(case.boxes[b]), dev(case.kps[b])
            lab = None if case.labels is None else dev(case.labels[b], np.int64)
            self.keep += [bb, kp, lab]
            t.num_gt[b] = len(case.boxes[b])
            t.gt_bboxes[b], t.gt_keypoints[b] = bb.data_ptr(), kp.data_ptr()
            t.gt_labels[b] = None if lab is None else lab.data_ptr()
            t.valid_h[b], t.valid_w[b] = case.valid[b]
        c = HL.HeadLossCfg()
        c.pos_num, c.pos_weight, c.normalize_term = case.pos_num, case.pos_weight, case.normalize_term
        for s in range(3):
            c.gamma[s], c.alpha[s] = case.gamma[s], case.alpha[s]
        for s in range(6):
            c.beta[s] = case.beta[s]
        for s in range(9):
            c.loss_weight[s] = case.loss_weight[s]
        self.t, self.c = t, c
        self.maps = [dev(m) for k in ('cls', 'bbox', 'kpt') for m in case.maps[k]]
        self.hm = HL._maps(self.maps)
        self.up = dev(np.asarray(case.upstream, np.float32))
        self.ws_bytes = L.kgdet_head_loss_workspace_bytes(ctypes.byref(t))
        self.ws = Guarded((self.ws_bytes + 3) // 4)
        self.out = Guarded(10)
        self.grads = [Guarded(m.numel()) for m in self.maps]
        hg = HL.HeadMaps()
        for s in range(3):
            hg.cls[s], hg.bbox[s], hg.kpt[s] = self.grads[s].ptr(), self.grads[3 + s].ptr(), self.grads[6 + s].ptr()
        self.hg = hg

    def forward(self, ws_bytes=None, maps=None, losses=True):
        lib, L = _L()
        return L.kgdet_head_loss_forward(ctypes.byref(self.t), ctypes.byref(self.c), ctypes.byref(maps or self.hm),
                                         ctypes.c_void_p(self.out.ptr() if losses else 0), ctypes.c_void_p(self.out.ptr() + 36),
                                         ctypes.c_void_p(self.ws.ptr()), ctypes.c_size_t(self.ws_bytes if ws_bytes is None else ws_bytes),
                                         lib.current_stream())

    def backward(self, ws_bytes=None, grads=None):
        lib, L = _L()
        return L.kgdet_head_loss_backward(ctypes.byref(self.t), ctypes.byref(self.c), ctypes.byref(self.hm), ctypes.c_void_p(self.up.data_ptr()),
                                          ctypes.c_void_p(self.out.ptr() + 36), ctypes.byref(grads or self.hg), ctypes.c_void_p(self.ws.ptr()),
                                          ctypes.c_size_t(self.ws_bytes if ws_bytes is None else ws_bytes), lib.current_stream())

    def nothing_written(self):
        torch.cuda.synchronize()
        return self.out.untouched() and self.ws.untouched() and all(g.untouched() for g in self.grads)

    def selections(self):
        """the kernel's dsel rows of every image: the first B * 64 * N floats of the workspace, [b][g][i] with row stride 64"""
        case = self.case
        d = self.ws.view()[:case.B * R.MAX_GT * case.N].cpu().numpy().reshape(case.B, R.MAX_GT, case.N)
        return [d[b, :len(case.boxes[b])] for b in range(case.B)]


def _note(family, err, bar, tag):
    r = 0.0 if err == 0 else (float('inf') if bar == 0 else err / bar)
    WORST[family] = max(WORST.get(family, 0.0), r)
    print('%s: error %.3e, bar %.3e (%.3f of it); worst so far: %s' % (tag, err, bar, r, {k: round(v, 3) for k, v in WORST.items()}))
    return r


def _check_case(name):
    lib, L = _L()
    case = R.make_case(name)
    call = Call(case)
    lib.check(call.forward(), 'kgdet_head_loss_forward')
    lib.check(call.backward(), 'kgdet_head_loss_backward')
    torch.cuda.synchronize()
    out = call.out.view().cpu().numpy()
    first = [out.copy()] + [g.view().clone() for g in call.grads]
    dsel = call.selections()

    # 1. the selections are a correct assigner's; 3. and the reference's own where it decides
    assigned = []
    for b in range(case.B):
        D = case.distances(b)
        assigned.append(R.check_assignment(dsel[b], D, case.pos_num))
        if case.regime in ('decided', 'exact'):
            # 'exact': ties broken by the documented rule -- lowest point index (reference_selection's stable order), then the
            # earliest gt (assign_from_selection's first minimum)
            sel = R.reference_selection(D, case.pos_num)
            assert ((dsel[b] < np.inf) == sel).all(), 'image %d: not the reference selection' % b
            assert (assigned[b] == R.assign_from_selection(D, sel)).all(), 'image %d: not the reference assignment' % b
    # 2. num_total from the selections, exactly
    total = R.num_total(assigned)
    assert out[9] == total, (out[9], total)
    # 6. canaries, no NaN left
    assert call.out.intact() and call.ws.intact() and all(g.intact() for g in call.grads)
    assert np.isfinite(out).all()

    # 4. losses and gradients of the kernel's own assignment inside the bars; 5. the exact-zero patterns
    big = case.B * case.K * case.N > 4000000
    groups = [[k] for k in range(9)] if big else [list(range(9))]       # (the envelope case: one gradient map at a time)
    ref = R.losses_and_grads(case, assigned, grad_of=())
    res = R.losses_and_grads(case, assigned, f32=True, grad_of=())
    loss_bar, _ = R.bars(ref, res)
    worst = 0.0
    for k in range(9):
        fam = 'loss_' + R.KINDS[k // 3]
        worst = max(worst, _note(fam, abs(float(out[k]) - ref[0][k]), loss_bar[k], '%s loss %d' % (name, k)))
    if name == 'saturated_logits':
        # beyond |x| = 80 the float32 formula saturates (p = 0 -> log(FLT_MIN), as in the reference's CUDA code) and the bar above
        # is wide: there the kernel is ALSO held to the float32 restatement within the allowance tests/test_gpu_step_kernels.py
        # grants csrc/focal.hip, 1e-5 of the output
        for k in range(3):
            assert abs(float(out[k]) - float(res[0][k])) <= 1e-5 * abs(float(res[0][k])), (k, out[k], res[0][k])
    for ks in groups:
        r64 = R.losses_and_grads(case, assigned, grad_of=ks, want_losses=False)[2]
        r32 = R.losses_and_grads(case, assigned, f32=True, grad_of=ks, want_losses=False)[2]
        _, grad_bar = R.bars((ref[0], total, r64), (res[0], total, r32))
        for k in ks:
            got = call.grads[k].view().cpu().numpy().reshape(r64[k].shape)
            assert np.isfinite(got).all(), 'gradient map %d holds a NaN or an infinity' % k
            err = float(np.abs(got - r64[k]).max())
            worst = max(worst, _note('grad_' + R.KINDS[k // 3], err, grad_bar[k], '%s grad %d' % (name, k)))
            for b in range(case.B):
                inside = R.valid_mask(case.H, case.W, *case.extents(b))
                assert (got[b][:, ~inside] == 0).all(), 'map %d: a gradient outside the valid extent' % k
                if k >= 3:
                    assert (got[b][:, assigned[b] == 0] == 0).all(), 'map %d: a gradient at an unassigned point' % k
                if k >= 6:
                    vis = np.repeat(case.kps[b][:, :, 2] != 0, 2, axis=1)[np.maximum(assigned[b] - 1, 0)].T
                    assert (got[b][~vis] == 0).all(), 'map %d: a gradient at an invisible keypoint' % k
            zero_ref = r64[k] == 0
            assert (got[zero_ref] == 0).all(), 'map %d: non-zero where the reference is exactly zero' % k
        del r64, r32
    assert worst <= 1.0, 'an output is %.3f of its bar away' % worst

    # 7. a second forward + backward: the same bits
    call.ws.view().fill_(float('nan'))
    lib.check(call.forward(), 'kgdet_head_loss_forward')
    lib.check(call.backward(), 'kgdet_head_loss_backward')
    torch.cuda.synchronize()
    assert (call.out.view().cpu().numpy().view(np.int32) == first[0].view(np.int32)).all()
    for k in range(9):
        assert torch.equal(call.grads[k].view().view(torch.int32), first[1 + k].view(torch.int32)), k
    return case, call, assigned


@pytest.mark.parametrize('name', sorted(n for n, sp in R.CASES.items() if sp['regime'] == 'decided'))
def test_decided_case(name):
    """random inputs whose margins all exceed 64 M: the kernel's selections and assignment equal the float64 reference's, and
    every item of the list above holds (per case: tests/head_loss_refs.py CASES says which edge it is there for)"""
    _check_case(name)
    torch.cuda.empty_cache()


@pytest.mark.parametrize('name', sorted(n for n, sp in R.CASES.items() if sp['regime'] == 'exact'))
def test_exact_tie_case(name):
    """exact float32 ties: the lowest point index wins a tie at the cut, the earliest gt a tie for a point"""
    case, call, assigned = _check_case(name)
    if name == 'identical_64':
        assert set(np.unique(assigned[0])) == {0, 1} and (assigned[0] == 1).sum() == case.pos_num
    if name == 'exact_midcell_pos1':
        assert (assigned[0] > 0).sum() == 1 and int(np.flatnonzero(assigned[0])[0]) == 3 * case.W + 4     # the upper left of the four


@pytest.mark.parametrize('name', sorted(n for n, sp in R.CASES.items() if sp['regime'] == 'free'))
def test_near_tie_case(name):
    """near-ties on purpose: whatever the kernel selects must be a correct assigner's choice within M, and everything after the
    assignment -- num_total, losses, gradients, zero patterns, canaries, determinism -- follows from ITS choice"""
    case, call, assigned = _check_case(name)
    if name == 'inexact_tie':
        # which of the eight points (2, 1) / (1, 2) cells from the centre take ranks 13 .. 15 is the kernel's to choose; the torch
        # chain's float32 distances on the same device say what an uncontracted evaluation chooses -- printed, and held to the
        # same conditions
        from kgdet_amd import points
        pts = points.PointGenerator().grid_points((case.H, case.W), int(case.stride), device='cuda')
        chain = points.assign_points(pts, torch.from_numpy(case.boxes[0]).cuda(), 4, case.pos_num).cpu().numpy()
        R.check_assignment(chain, case.distances(0), case.pos_num)
        same = bool((chain == assigned[0]).all())
        print('inexact tie: kernel %s, torch chain %s: %s' % (np.flatnonzero(assigned[0]).tolist(), np.flatnonzero(chain).tolist(),
                                                               'the same points' if same else 'DIFFERENT points'))


# ============================================================================================ status codes
def _small():
    return R.make_case('n35_c1k1')


@pytest.mark.parametrize('what', ['B0', 'B17', 'gt0', 'gt65', 'points4097', 'pos_num_beyond_valid', 'pos_num_beyond_N', 'beta0',
                                  'beta_negative', 'null_map', 'null_grad', 'null_losses'])
def test_rejected_arguments_write_nothing(what):
    lib, L = _L()
    from kgdet_amd import head_loss as HL
    call = Call(_small())
    maps = grads = None
    if what == 'B0':
        call.t.B = 0
    elif what == 'B17':
        call.t.B = 17
    elif what == 'gt0':
        call.t.num_gt[0] = 0
    elif what == 'gt65':
        call.t.num_gt[0] = 65
    elif what == 'points4097':
        call.t.H, call.t.W = 17, 241
    elif what == 'pos_num_beyond_valid':
        call.t.valid_h[0], call.t.valid_w[0] = 2, 4
    elif what == 'pos_num_beyond_N':
        call.c.pos_num = 36
    elif what == 'beta0':
        call.c.beta[4] = 0.0
    elif what == 'beta_negative':
        call.c.beta[1] = -0.5
    elif what == 'null_map':
        maps = HL._maps(call.maps)
        maps.kpt[1] = None
    elif what == 'null_grad':
        grads = HL.HeadMaps()
        for s in range(3):
            grads.cls[s], grads.bbox[s], grads.kpt[s] = call.hg.cls[s], call.hg.bbox[s], call.hg.kpt[s]
        grads.bbox[2] = None
    if what != 'null_grad':
        assert call.forward(maps=maps, losses=what != 'null_losses') == lib.KGDET_E_SHAPE
    if what not in ('null_map', 'null_losses'):
        assert call.backward(grads=grads) == lib.KGDET_E_SHAPE
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
    assert call.ws.intact()                       # the size kgdet_head_loss_workspace_bytes names is enough


# ============================================================================================ the wrapper
def _head_inputs(B, n_gt, seed=0):
    from kgdet_amd import configs
    from kgdet_amd.registry import build_head
    cfg = configs.kgdet_r50_fpn()
    cfg.train_cfg.uniform.assigner['pos_num'] = 3
    torch.manual_seed(seed)
    head = build_head(cfg.model.bbox_head).cuda()
    g = torch.Generator().manual_seed(seed + 1)
    H, W, K = 5, 7, 294
    gt_b, gt_l, gt_k = [], [], []
    for b in range(B):
        n = n_gt[b]
        xy = torch.rand(n, 2, generator=g) * torch.tensor([200., 140.]) + 10
        wh = torch.rand(n, 2, generator=g) * 100 + 40
        gt_b.append(torch.cat([xy - wh / 2, xy + wh / 2], 1).cuda())
        gt_k.append(torch.cat([torch.rand(n, K, 2, generator=g) * 150, (torch.rand(n, K, 1, generator=g) < 0.2).float() * 2], 2).cuda())
        gt_l.append(torch.randint(1, 14, (n,), generator=g).cuda())
    metas = [dict(pad_shape=(160, 224, 3), img_shape=(160, 224, 3), scale_factor=1.0, flip=False)] * B

    def run(fused):
        from kgdet_amd import head_loss
        gg = torch.Generator().manual_seed(seed + 2)
        mk = lambda c, s: (torch.randn(B, c, H, W, generator=gg) * s).cuda().requires_grad_()
        cls, kpt, bbox = ([[mk(13, 2.0)] for _ in range(3)], [[mk(2 * K, 4.0)] for _ in range(3)], [[mk(4, 4.0)] for _ in range(3)])
        prev = head_loss.ENABLED
        head_loss.ENABLED = fused
        try:
            losses = head.loss(cls[0], cls[1], cls[2], kpt[0], kpt[1], kpt[2], bbox[0], bbox[1], bbox[2], gt_b, gt_l, gt_k, metas,
                               cfg.train_cfg)
        finally:
            head_loss.ENABLED = prev
        sum(sum(v) for v in losses.values()).backward()
        return {n: float(sum(v)) for n, v in losses.items()}, [m[0].grad.clone() for grp in (cls, kpt, bbox) for m in grp]
    return run


@pytest.mark.parametrize('B,n_gt', [(17, [1] * 17), (2, [65, 1])])
def test_wrapper_falls_back_beyond_the_envelope(B, n_gt, monkeypatch):
    """17 images, or 65 gts in one image: head.loss takes the torch chain (the fused entry is never reached) and returns what the
    chain returns with the fused path switched off"""
    from kgdet_amd import head_loss
    run = _head_inputs(B, n_gt)
    want_l, want_g = run(False)

    def never(*a, **k):
        raise AssertionError('the fused head loss was called beyond its envelope')
    monkeypatch.setattr(head_loss, 'head_loss', never)
    got_l, got_g = run(True)
    assert got_l == want_l and all(np.isfinite(v) for v in got_l.values())
    assert all(torch.equal(a, b) for a, b in zip(got_g, want_g))


@pytest.mark.parametrize('fused', [True, False])
def test_wrapper_raises_without_ground_truth(fused):
    run = _head_inputs(2, [2, 0])
    with pytest.raises(ValueError, match='No gt or bboxes'):
        run(fused)
