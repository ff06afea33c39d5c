"""The fused loss route of the serial / parallel heads (kgdet_amd/serial_loss.py behind _RepPointsHeadKpTwoStage.loss): when it
applies, that it replaces the torch target path, that both routes give the float64 reference's numbers on the same batch, that
every condition of ``applicable`` falls back to the torch chain, and that a config-5 training step stays free of host syncs."""
import copy

import numpy as np
import pytest
import torch

from kgdet_amd import configs
from tests import head_loss_refs as H
from tests import serial_loss_refs as R
from tests.golden import ref_cases

pytestmark = pytest.mark.gpu
f32 = np.float32


def _golden(parallel):
    cfg = configs.reppoints_kp_r50_fpn(parallel=parallel)
    head = ref_cases.serial_head(parallel=parallel).cuda()
    head.train()
    xs, batch = ref_cases.serial_inputs((256, 320))
    return cfg, head, xs, batch


def _gt(batch):
    to = lambda l: [t.cuda() for t in l]
    return to(batch['gt_bboxes']), to(batch['gt_labels']), to(batch['gt_keypoints'])


@pytest.mark.parametrize('parallel', [False, True])
def test_route_applies_and_replaces_the_torch_target_path(parallel, monkeypatch):
    from kgdet_amd import heads_serial, points, serial_loss
    cfg, head, xs, batch = _golden(parallel)
    outs = head([x.cuda() for x in xs], batch['img_meta'])
    gt = _gt(batch)
    assert serial_loss.ENABLED
    assert serial_loss.applicable(head, cfg.train_cfg, *outs, *gt, batch['img_meta'], None)

    def never(*a, **k):
        raise AssertionError('the torch target path was called with the fused route on')
    for mod in (points, heads_serial):
        monkeypatch.setattr(mod, 'point_target_kp_dense', never)
        monkeypatch.setattr(mod, 'point_target_kp', never)
    losses = head.loss(*outs, *gt, batch['img_meta'], cfg.train_cfg)
    assert sorted(losses) == sorted(R.NAMES)
    for v in losses.values():
        assert len(v) == 5 and all(t.dim() == 0 and bool(torch.isfinite(t)) for t in v)
    sum(sum(v) for v in losses.values()).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in head.parameters())


def _case_of(head, cfg, outs, box_init, box_refine, batch):
    n = lambda maps: [m.detach().cpu().numpy().astype(f32) for m in maps]
    a = cfg.train_cfg.refine.assigner
    cls, kpt_i, kpt_r = outs[0], outs[1], outs[2]
    return R.Case(name='golden', B=cls[0].shape[0], C=head.cls_out_channels, K=head.num_keypts,
                  strides=[float(s) for s in head.point_strides], shapes=[tuple(m.shape[-2:]) for m in cls],
                  valid=[[(0, 0)] * len(cls)] * cls[0].shape[0], boxes=[b.numpy() for b in batch['gt_bboxes']],
                  kps=[k.numpy() for k in batch['gt_keypoints']], labels=[l.numpy() for l in batch['gt_labels']],
                  pos_num=cfg.train_cfg.init.assigner['pos_num'], upstream=np.ones(5 * len(cls), f32), pos_weight=1.0,
                  gamma=head.loss_cls.gamma, alpha=head.loss_cls.alpha, beta=[getattr(head, m).beta for m in R.NAMES[1:]],
                  loss_weight=[getattr(head, m).loss_weight for m in R.NAMES], pos_iou_thr=a['pos_iou_thr'], neg_lo=0.0,
                  neg_hi=a['neg_iou_thr'], min_pos_iou=a['min_pos_iou'], scale=4.0, point_base_scale=float(head.point_base_scale),
                  maps=dict(cls=n(cls), box_init=n(box_init), box_refine=n(box_refine), kpt_init=n(kpt_i), kpt_refine=n(kpt_r)))


@pytest.mark.parametrize('parallel', [False, True])
def test_both_routes_give_the_float64_reference(parallel, monkeypatch):
    """Same head, same batch, route on and off.
    Assignments: the fused route's (read from the workspace of a C ABI call on the same maps) equal the numpy reference's, and the
    torch route's targets (point_target_kp_dense's labels, label weights and gathered boxes, recorded) say the same.
    Losses: each route inside serial_loss_refs.bars of the float64 reference on ITS inputs: the head's maps and, for the boxes,
    the fused route's moment-box maps / the torch route's moment box of the decoded points (restated exactly as a float64 box map).
    Gradients of every head parameter and of the pyramid inputs: the bar carried through the linear backward behind the maps --
    the float64 reference's and the float32 restatement's map gradients are both pushed through the same network (for the torch
    route through ITS box graph), and a route's gradient must lie within 4 x their difference of the former, floored at 6
    roundings of the tensor's scale.  The worst fraction per route is printed and asserted."""
    from kgdet_amd import heads_serial, serial_loss
    from tests.test_gpu_serial_loss_kernels import Call
    cfg, head, xs_cpu, batch = _golden(parallel)
    gt = _gt(batch)
    recorded = []
    original = heads_serial.point_target_kp_dense

    def recording(*a, **k):
        out = original(*a, **k)
        recorded.append(out)
        return out
    monkeypatch.setattr(heads_serial, 'point_target_kp_dense', recording)

    def run(fused):
        monkeypatch.setattr(serial_loss, 'ENABLED', fused)
        head.zero_grad()
        xs = [x.clone().cuda().requires_grad_() for x in xs_cpu]
        outs = head(xs, batch['img_meta'])
        losses = head.loss(*outs, *gt, batch['img_meta'], cfg.train_cfg)
        return xs, outs, losses

    # the reference, from the head's maps
    xs, outs, losses = run(True)
    assert not recorded
    with torch.no_grad():
        box_i, box_r = [head.points2bbox(r) for r in outs[3]], [head.points2bbox(r) for r in outs[4]]
    case = _case_of(head, cfg, outs, box_i, box_r, batch)
    call = Call(case)
    assert call.forward() == 0
    torch.cuda.synchronize()
    ai, ar, _ = call.assignments()
    for b in range(case.B):
        assert (ai[b] == R.init_reference(case, b)).all() and (ar[b] == R.refine_reference(case, b)[0]).all()
    ref = R.losses_and_grads(case, list(ai), list(ar))

    def check_losses(losses, tag, ref, loss_bar):
        worst = 0.0
        for k, name in enumerate(R.NAMES):
            got = np.array([float(t.detach()) for t in losses[name]])
            for l in range(case.L):
                err, bar = abs(got[l] - ref[0][k, l]), loss_bar[k, l]
                r = 0.0 if err == 0 else (np.inf if bar == 0 else err / bar)
                worst = max(worst, r)
                print('%s %s level %d: error %.3e, bar %.3e (%.3f of it)' % (tag, name, l, err, bar, r))
        print('%s: worst loss at %.3f of its bar' % (tag, worst))
        assert worst <= 1.0, '%s: a loss is %.3f of its bar away' % (tag, worst)

    def grads_of(xs):
        return [p.grad.clone() for p in head.parameters()] + [x.grad.clone() for x in xs]

    def pushed(table, chain):
        """the map gradients ``table`` ((family, level) -> [B, ch, Nl], numpy) through the network behind the maps, on a forward
        of its own (one backward per graph): gradients of every head parameter and pyramid input.  ``chain``: the boxes enter as
        the torch chain forms them -- the moment box of the DECODED points, image space, [B * Nl, 4]"""
        xs_, outs_, _ = run(True)
        dev = lambda k, l: torch.from_numpy(np.ascontiguousarray(table[(k, l)]).astype(f32)).cuda()
        if chain:
            boxes = _chain_boxes(head, outs_[3], batch['img_meta']) + _chain_boxes(head, outs_[4], batch['img_meta'])
            box_up = lambda k, l: (dev(k, l) / case.strides[l]).permute(0, 2, 1).reshape(-1, 4)
        else:
            boxes = _boxes_of(head, outs_[3]) + _boxes_of(head, outs_[4])
            box_up = lambda k, l: dev(k, l).reshape(boxes[0].shape[0], 4, *case.shapes[l])
        tensors = list(outs_[0]) + boxes + list(outs_[1]) + list(outs_[2])
        ups = [box_up(k, l) if k in (1, 2) else dev(k, l).reshape(tensors[k * case.L + l].shape)
               for k in range(5) for l in range(case.L)]
        got = torch.autograd.grad(tensors, list(head.parameters()) + xs_, grad_outputs=ups, allow_unused=True)
        return [None if g is None else g.double().cpu().numpy() for g in got]

    names = [n for n, _ in head.named_parameters()] + ['x%d' % l for l in range(len(xs))]

    def check_grads(got, ref64, res32, tag):
        """the bar carried through the (linear) backward behind the maps: per tensor 4 x the difference between the float32
        restatement's and the float64 reference's map gradients pushed through the same network, floored at the kernels' largest
        floor of roundings of the tensor's scale"""
        want, want32 = pushed(ref64[2], tag == 'torch chain'), pushed(res32[2], tag == 'torch chain')
        worst, where = 0.0, None
        for n, g, w, w32 in zip(names, got, want, want32):
            g = g.double().cpu().numpy()
            w = np.zeros_like(g) if w is None else w
            w32 = np.zeros_like(g) if w32 is None else w32
            scale = float(np.abs(w).max())
            bar = 4 * max(float(np.abs(w32 - w).max()), max(R.FLOOR.values()) * R.U * scale)
            err = float(np.abs(g - w).max())
            r = 0.0 if err == 0 else (np.inf if bar == 0 else err / bar)
            print('%s grad %s: error %.3e, bar %.3e (%.3f of it), scale %.3e' % (tag, n, err, bar, r, scale))
            if r > worst:
                worst, where = r, n
        print('%s: worst parameter / input gradient at %.3f of its bar (%s)' % (tag, worst, where))
        assert worst <= 1.0, '%s: the gradient of %s is %.3f of its bar away' % (tag, where, worst)

    res = R.losses_and_grads(case, list(ai), list(ar), f32=True)
    check_losses(losses, 'fused', ref, R.bars(ref, res)[0])
    sum(sum(v) for v in losses.values()).backward()
    check_grads(grads_of(xs), ref, res, 'fused')

    # the torch chain: the same assignments, and the float64 reference of ITS inputs -- its box is the moment box of the decoded
    # points (image space), restated here as the box map (box - centre) / stride in float64, which reproduces it exactly
    xs2, outs2, losses2 = run(False)
    assert len(recorded) == 2                                       # init, then refine
    off = case.offsets
    for stage, a in ((0, ai), (1, ar)):
        labels, label_w, bbox_gt = recorded[stage][0], recorded[stage][1], recorded[stage][2]
        for l in range(case.L):
            for b in range(case.B):
                mine = a[b][off[l]:off[l + 1]]
                assert ((labels[l][b].cpu().numpy() > 0) == (mine > 0)).all()
                assert (labels[l][b].cpu().numpy() == np.where(mine > 0, case.labels[b][np.maximum(mine - 1, 0)], 0)).all()
                assert (label_w[l][b].cpu().numpy() == np.where(mine > 0, 1.0, (mine == 0) * 1.0)).all()
                assert (bbox_gt[l][b].cpu().numpy() == np.where((mine > 0)[:, None], case.boxes[b][np.maximum(mine - 1, 0)], 0)).all()
    case2 = copy.copy(case)
    case2.maps = dict(case.maps)
    with torch.no_grad():
        for name, reppts in (('box_init', outs2[3]), ('box_refine', outs2[4])):
            maps = []
            for l, box in enumerate(_chain_boxes(head, reppts, batch['img_meta'])):
                h, w = case.shapes[l]
                px, py = (a.astype(np.float64) for a in H.grid_points(case.strides[l], h, w))
                img = box.double().cpu().numpy().reshape(case.B, h * w, 4).transpose(0, 2, 1)
                raw = (img - np.stack([px, py, px, py])[None]) / case.strides[l]
                assert (raw * case.strides[l] + np.stack([px, py, px, py])[None] == img).all()
                maps.append(raw.reshape(case.B, 4, h, w))
            case2.maps[name] = maps
    ref2 = R.losses_and_grads(case2, list(ai), list(ar))
    res2 = R.losses_and_grads(case2, list(ai), list(ar), f32=True)
    check_losses(losses2, 'torch chain', ref2, R.bars(ref2, res2)[0])
    sum(sum(v) for v in losses2.values()).backward()
    check_grads(grads_of(xs2), ref2, res2, 'torch chain')


def _chain_boxes(head, reppts, metas):
    """the boxes as the torch chain forms them, attached to the graph of ``reppts``: per level the moment box [B * Nl, 4] of the
    decoded points, image space (heads_serial loss / loss_single)"""
    centers, _ = head.get_points([r.shape[-2:] for r in reppts], metas, device=reppts[0].device)
    return [head.points2bbox(p.reshape(-1, p.shape[-1]), y_first=False) for p in head.offset_to_pts(centers, reppts)]


def _boxes_of(head, reppts):
    """the box maps as the fused route forms them, attached to the graph of ``reppts``"""
    return [head.points2bbox(r) for r in reppts]


# ============================================================================================ fallbacks
def _loss_inputs(seed=0):
    """random maps on the 256 x 320 pyramid as leaves (no towers): enough for head.loss"""
    cfg, head, _, batch = _golden(False)
    g = torch.Generator().manual_seed(seed)
    shapes = R.pyramid(256, 320)
    mk = lambda ch, sc: [(torch.randn(2, ch, h, w, generator=g) * sc).cuda().requires_grad_() for h, w in shapes]
    maps = (mk(13, 2.0), mk(588, 1.0), mk(588, 1.0), mk(18, 2.0), mk(18, 2.0))
    return cfg, head, maps, batch


def _numbers(head, maps, gt, metas, train_cfg, **kw):
    losses = head.loss(*maps, *gt, metas, train_cfg, **kw)
    return {k: [float(t.detach()) for t in v] for k, v in losses.items()}


@pytest.mark.parametrize('what', ['autocast', 'gt_bboxes_ignore', 'pos_scale_factor', 'gt_max_assign_all_false', 'cpu_ground_truth',
                                  'switched_off'])
def test_fallback_returns_the_torch_chain(what, monkeypatch):
    import contextlib
    from kgdet_amd import serial_loss
    cfg, head, maps, batch = _loss_inputs()
    gt = list(_gt(batch))
    train_cfg = configs.reppoints_kp_r50_fpn().train_cfg
    kw = {}
    ctx = contextlib.nullcontext
    assert serial_loss.applicable(head, train_cfg, *maps, *gt, batch['img_meta'], None)
    if what == 'autocast':
        ctx = lambda: torch.autocast('cuda', dtype=torch.bfloat16)
    elif what == 'gt_bboxes_ignore':
        kw['gt_bboxes_ignore'] = [torch.tensor([[10., 10., 60., 60.]]).cuda()] * 2
    elif what == 'pos_scale_factor':
        train_cfg.init.assigner['pos_scale_factor'] = 0.4
    elif what == 'gt_max_assign_all_false':
        train_cfg.refine.assigner['gt_max_assign_all'] = False
    elif what == 'cpu_ground_truth':
        gt[0] = [t.cpu() for t in gt[0]]
    elif what == 'switched_off':
        monkeypatch.setattr(serial_loss, 'ENABLED', False)

    def fused_never(*a, **k):
        raise AssertionError('the fused route was taken')
    with ctx():
        assert not serial_loss.applicable(head, train_cfg, *maps, *gt, batch['img_meta'], kw.get('gt_bboxes_ignore'))

    def outcome():
        try:
            with ctx():
                return _numbers(head, maps, gt, batch['img_meta'], train_cfg, **kw)
        except RuntimeError as e:             # (CPU ground truth against CUDA maps: torch's own device-mismatch error)
            return type(e)
    want = None
    if what != 'switched_off':
        monkeypatch.setattr(serial_loss, 'ENABLED', False)
        want = outcome()
        monkeypatch.setattr(serial_loss, 'ENABLED', True)
    monkeypatch.setattr(serial_loss, 'serial_loss', fused_never)
    got = outcome()
    if want is not None:
        assert got == want
    if what != 'cpu_ground_truth':
        assert isinstance(got, dict) and all(np.isfinite(v).all() for v in got.values())


# ============================================================================================ the training step
def test_config5_step_runs_on_the_fused_route_without_host_syncs(monkeypatch):
    from kgdet_amd import serial_loss, synthetic
    from kgdet_amd.dist import DistOptimizerHook
    from kgdet_amd.registry import build_detector
    cfg = configs.reppoints_kp_r50_fpn()
    torch.manual_seed(0)
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda()
    batch = synthetic.make_batch(2, 'cuda', seed=0, img_shape=(256, 320, 3), pad_shape=(256, 320, 3))
    for k in ('gt_bboxes', 'gt_keypoints'):
        batch[k] = [t.clamp(max=250) for t in batch[k]]
    model.train()
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-6, momentum=0.9, fused=True)
    hook = DistOptimizerHook(grad_clip=dict(max_norm=35, norm_type=2))
    calls = []
    fused = serial_loss.serial_loss
    monkeypatch.setattr(serial_loss, 'serial_loss', lambda *a, **k: (calls.append(1), fused(*a, **k))[1])

    def step():
        losses = model(batch['img'], batch['img_meta'], return_loss=True, gt_bboxes=batch['gt_bboxes'],
                       gt_labels=batch['gt_labels'], gt_keypoints=batch['gt_keypoints'])
        total = sum(sum(v) if isinstance(v, (list, tuple)) else v for v in losses.values())
        hook.step(model, opt, total)
        return total

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        total = step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert len(calls) == 3 and bool(torch.isfinite(total))
