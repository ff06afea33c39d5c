"""The ResNeXt backbone on the GPU: the small net of tests/resnext_cases.py with the grouped route on against the route off
(torch's grouped convolution), both against a float64 CPU run of the same module; inference in fp32 (fused bias + ReLU store)
and under bf16 autocast (stays on torch); bit repeatability; one training step and one detection pass of a KGDet detector on a
ResNeXt-50 32x4d."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import resnext_cases as X
from tests.dense_refs import ACC_BAR

pytestmark = pytest.mark.gpu

INPUT = (2, 3, 64, 96)
GROUPED = 7          # grouped conv2 of the small net: 3 in layer1 (frozen: no weight gradient), 4 in layer2
TRAINABLE = 4
# the detector's synthetic batch: 2 x 160 x 192, a 5 x 6 grid at stride 32.  (2 x 128 x 160 has 4 x 5 = 20 points, fewer than the
# PointAssigner's pos_num = 25 of the KGDet config: its top-k cannot run on any backbone.)
IMG = (160, 192, 3)
BF16_BAR = 0.05      # of the fp32 features' max: the bar of test_gpu_backbone's bf16 inference comparison


@pytest.fixture(autouse=True)
def forced_route(monkeypatch):
    """the correctness tests run the route whatever the default of a shape class is"""
    from kgdet_amd import backbone, conv1x1, grouped_conv
    monkeypatch.setattr(grouped_conv, 'FORCE', True)
    monkeypatch.setattr(grouped_conv, 'ENABLED', True)
    conv1x1._entries.clear(), conv1x1._fold_entries.clear()
    backbone.clear_fold_cache()
    yield
    conv1x1._entries.clear(), conv1x1._fold_entries.clear()
    backbone.clear_fold_cache()


def _small(style='pytorch'):
    from kgdet_amd.backbone import ResNeXt
    return X.fill(ResNeXt(style=style, **X.SMALL))


def _cotangents(outs):
    """formula cotangents of the outputs (no RNG), as float64 CPU tensors"""
    gs = []
    for k, o in enumerate(outs):
        i = torch.arange(o.numel(), dtype=torch.float64)
        gs.append((torch.cos(0.37 * i + k) + 0.25 * torch.sin(0.011 * i)).reshape(o.shape))
    return gs


@pytest.fixture(scope='module')
def reference():
    """the float64 CPU run of the small net in train mode: outputs, the gradient of every trainable parameter and of the input"""
    net = _small().double()
    net.train()
    x = X.formula_input(INPUT).requires_grad_(True)
    outs = net(x)
    gs = _cotangents(outs)
    torch.autograd.backward(outs, gs)
    grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    grads['input'] = x.grad.clone()
    return [o.detach() for o in outs], grads, gs


def _train_pass(net, gs, steps=1):
    """``steps`` training passes inside conv1x1.step_scope (the second one runs the folded nodes with their gate links);
    the last pass's outputs and gradients"""
    from kgdet_amd import conv1x1
    for _ in range(steps):
        net.zero_grad(set_to_none=True)
        x = X.formula_input(INPUT, torch.float32).cuda().requires_grad_(True)
        with conv1x1.step_scope():
            outs = net(x)
        torch.autograd.backward(outs, [g.float().cuda() for g in gs])
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    grads['input'] = x.grad.detach().clone()
    return [o.detach() for o in outs], grads


def _err(got, want):
    return float((got.double().cpu() - want).abs().max())


def _hold(tag, new, old, want):
    """the new route's error at most 4 x the torch route's on this tensor, floor ACC_BAR of the tensor's max"""
    e_new, e_old, scale = _err(new, want), _err(old, want), float(want.abs().max())
    bar = max(4 * e_old, ACC_BAR * scale)
    print('%s: route %.3g, torch %.3g of the max; %.3f of the bar' % (tag, e_new / scale, e_old / scale, e_new / bar))
    assert np.isfinite(e_new) and e_new <= bar, tag


@pytest.mark.parametrize('steps', [1, 2], ids=['unfolded', 'folded'])
def test_training_routes_against_float64(reference, steps, monkeypatch):
    from kgdet_amd import grouped_conv as G
    want_outs, want_grads, gs = reference
    net = _small().cuda()
    net.train()
    G.reset_calls()
    new_outs, new_grads = _train_pass(net, gs, steps)
    # every grouped conv2 took the route: forward and grad_input in both stages (the input asks for its gradient), the weight
    # gradient in the trainable stage
    assert G.calls == dict(forward=GROUPED * steps, bias_act=0, grad_input=GROUPED * steps, grad_weight=TRAINABLE * steps)
    monkeypatch.setattr(G, 'ENABLED', False)
    G.reset_calls()
    old_outs, old_grads = _train_pass(net, gs, steps)
    assert not any(G.calls.values())
    assert set(new_grads) == set(old_grads) == set(want_grads)
    assert sum(1 for n in new_grads if n.endswith('conv2.weight')) == TRAINABLE
    for i in range(2):
        _hold('output %d' % i, new_outs[i], old_outs[i], want_outs[i])
    for n in sorted(want_grads):
        _hold('grad ' + n, new_grads[n], old_grads[n], want_grads[n])


@pytest.mark.parametrize('style', X.STYLES)
def test_fp32_inference_takes_the_fused_store(style, monkeypatch):
    from kgdet_amd import backbone, grouped_conv as G
    net = _small(style)
    ref = copy.deepcopy(net).double()
    ref.eval()
    with torch.no_grad():
        want = ref(X.formula_input(INPUT))
    net = net.cuda()
    net.eval()
    x = X.formula_input(INPUT, torch.float32).cuda()
    G.reset_calls()
    with torch.no_grad():
        new = net(x)
    assert G.calls == dict(forward=0, bias_act=GROUPED, grad_input=0, grad_weight=0)
    monkeypatch.setattr(G, 'ENABLED', False)
    backbone.clear_fold_cache()
    G.reset_calls()
    with torch.no_grad():
        old = net(x)
    assert not any(G.calls.values())
    for i in range(2):
        _hold('%s eval output %d' % (style, i), new[i], old[i], want[i])


def test_bf16_autocast_inference_stays_on_torch_and_is_finite():
    from kgdet_amd import grouped_conv as G
    net = _small().cuda()
    net.eval()
    x = X.formula_input(INPUT, torch.float32).cuda()
    with torch.no_grad():
        ref = net(x)
        G.reset_calls()
        with torch.autocast('cuda', dtype=torch.bfloat16):
            for _ in range(3):          # (the measured 1x1 route choices settle in the first calls)
                got = net(x)
    assert not any(G.calls.values())
    for g, r in zip(got, ref):
        assert g.shape == r.shape and bool(torch.isfinite(g.float()).all())
        assert float((g.float() - r).abs().max()) <= BF16_BAR * float(r.abs().max())


def test_two_training_passes_give_equal_bits(reference):
    gs = reference[2]
    net = _small().cuda()
    net.train()
    _train_pass(net, gs, 2)
    a_outs, a = _train_pass(net, gs, 1)
    b_outs, b = _train_pass(net, gs, 1)
    for u, v in zip(a_outs, b_outs):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    for n in a:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n


@pytest.mark.parametrize('groups,planes', [(8, 64), (8, 128), (32, 64)], ids=['8x4', '8x8', '32x4'])
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('modulated', [False, True], ids=['v1', 'v2'])
def test_resnext_bottleneck_dcn_matches_the_grid_sample_reference(modulated, stride, groups, planes):
    """The ResNeXt block hands dcn['groups'] to its deformable conv2 (widths 32, 64 and 128: Cg = 4, 8 and 4): forward and every
    gradient of the block against the grid_sample formulation (tests/torch_ref.py, ``groups=groups``) on a float64 copy of the
    block, at the bars of test_gpu_backbone.py::test_bottleneck_dcn_option_matches_torch_reference."""
    from kgdet_amd import backbone as bb
    from tests import torch_ref
    torch.manual_seed(3)
    inplanes, outplanes, width = 64, 4 * planes, planes * 4 // 64 * groups
    down = nn.Sequential(nn.Conv2d(inplanes, outplanes, 1, stride=stride, bias=False), nn.BatchNorm2d(outplanes))
    blk = bb.ResNeXtBottleneck(inplanes, planes, stride=stride, downsample=down, groups=groups, base_width=4,
                               dcn=dict(modulated=modulated, groups=groups, deformable_groups=1, fallback_on_stride=False)).cuda()
    assert type(blk.conv2).__name__ == ('ModulatedDeformConv' if modulated else 'DeformConv')
    assert blk.conv2.groups == groups and tuple(blk.conv2.weight.shape) == (width, width // groups, 3, 3)
    assert blk.conv2_offset.out_channels == (27 if modulated else 18)
    for m in blk.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    blk.eval()            # norm_eval
    blk.conv2_offset.weight.data.normal_(0, 0.05)
    x0 = torch.randn(2, inplanes, 20, 28, device='cuda')
    ref = copy.deepcopy(blk).double().cpu()

    def reference(x):
        out = ref.relu(ref.norm1(ref.conv1(x)))
        om = ref.conv2_offset(out)
        if modulated:
            off, mask = om[:, :18], om[:, -9:].sigmoid()
        else:
            off, mask = om, None
        out = torch_ref.deform_conv(out, off, ref.conv2.weight, stride=stride, padding=1, dilation=1, groups=groups, mask=mask)
        if modulated and ref.conv2.bias is not None:
            out = out + ref.conv2.bias.view(1, -1, 1, 1)
        out = ref.relu(ref.norm2(out))
        out = ref.norm3(ref.conv3(out))
        return ref.relu(out + ref.downsample(x))

    def run(module, fn, x0):
        module.zero_grad()
        x = x0.clone().requires_grad_(True)
        y = fn(x)
        y.square().mean().backward()
        return y.detach(), x.grad, {n: p.grad.clone() for n, p in module.named_parameters() if p.grad is not None}

    y, gx, gp = run(blk, blk, x0)
    yr, gxr, gpr = run(ref, reference, x0.double().cpu())
    rel = lambda a, b: (a.double().cpu() - b).abs().max().item() / (b.abs().max().item() + 1e-12)
    tag = 'RESNEXT-DCN %s stride %d %dx%d' % ('v2' if modulated else 'v1', stride, groups, width // groups)
    assert y.shape == (2, outplanes, 20 // stride, 28 // stride)
    print('%s: output %.3g (bar 1e-4), grad x %.3g (bar 1e-3)' % (tag, rel(y, yr), rel(gx, gxr)))
    assert bool(torch.isfinite(y).all()) and rel(y, yr) <= 1e-4
    assert bool(torch.isfinite(gx).all()) and rel(gx, gxr) <= 1e-3
    assert gp.keys() == gpr.keys() and 'conv2_offset.weight' in gp and 'conv2.weight' in gp
    for n in gp:
        print('%s: grad %s %.3g (bar 1e-3)' % (tag, n, rel(gp[n], gpr[n])))
        assert bool(torch.isfinite(gp[n]).all()) and rel(gp[n], gpr[n]) <= 1e-3, n


def test_small_resnext_with_a_dcn_stage_steps_and_repeats():
    """the small net with layer2's conv2 deformable in 8 weight groups of 8 channels (dcn['groups'] = 8, width 64), every parameter --
    the conv2_offset weights too -- from the formulas of tests/resnext_cases.py: one training pass gives finite outputs and a
    finite non-zero gradient for every deformable conv2 and its offset convolution, and a second pass the same bits"""
    from kgdet_amd.backbone import ResNeXt
    net = X.fill(ResNeXt(style='pytorch', dcn=dict(modulated=False, groups=8, deformable_groups=1, fallback_on_stride=False),
                         stage_with_dcn=(False, True), **X.SMALL)).cuda()
    net.train()
    blocks = list(net.layer2)
    assert blocks and all(type(b.conv2).__name__ == 'DeformConv' and b.conv2.groups == 8 for b in blocks)
    assert not any(hasattr(b, 'conv2_offset') for b in net.layer1)
    assert all(float(b.conv2_offset.weight.abs().max()) > 0 for b in blocks), 'the offset convolutions must not be zero'
    with torch.no_grad():
        gs = _cotangents(net(X.formula_input(INPUT, torch.float32).cuda()))
    # (as in test_two_training_passes_give_equal_bits: the dense nodes of layer1 run unfolded in the first pass of a net and folded
    # from the second on, with other bits; the two passes compared are both of the settled kind)
    _train_pass(net, gs, 2)
    a_outs, a = _train_pass(net, gs)
    b_outs, b = _train_pass(net, gs)
    assert len(a_outs) == 2 and all(bool(torch.isfinite(o).all()) for o in a_outs)
    watched = [n for n in a if n.startswith('layer2.') and (n.endswith('.conv2.weight') or n.endswith('.conv2_offset.weight'))]
    assert len(watched) == 2 * len(blocks), watched
    for n in watched:
        assert bool(torch.isfinite(a[n]).all()) and float(a[n].abs().max()) > 0, n
    for u, v in zip(a_outs, b_outs):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    assert set(a) == set(b)
    for n in a:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n


@pytest.fixture(scope='module')
def detector():
    from kgdet_amd import configs
    from kgdet_amd.registry import build_detector
    cfg = configs.kgdet_x101_fpn(depth=50)
    torch.manual_seed(0)
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda()
    # zero_init_residual leaves every bottleneck's last BatchNorm at zero: no gradient would reach conv2 at all
    for m in model.backbone.modules():
        if hasattr(m, 'norm3'):
            nn.init.constant_(m.norm3.weight, 0.5)
    return cfg, model


def test_detector_training_step(detector):
    from kgdet_amd import grouped_conv as G, synthetic
    cfg, model = detector
    model.train()
    batch = synthetic.make_batch(2, 'cuda', seed=0, img_shape=IMG, pad_shape=IMG)
    G.reset_calls()
    losses = model(batch['img'], batch['img_meta'], return_loss=True, gt_bboxes=batch['gt_bboxes'],
                   gt_labels=batch['gt_labels'], gt_keypoints=batch['gt_keypoints'])
    values = [v for k, vs in losses.items() if 'loss' in k for v in (vs if isinstance(vs, (list, tuple)) else [vs])]
    assert len(values) == 9 and all(bool(torch.isfinite(v).all()) for v in values)
    sum(v.sum() for v in values).backward()
    blocks = [m for m in model.backbone.modules() if hasattr(m, 'conv2')]
    assert len(blocks) == 16 and G.calls['forward'] == 16
    trainable = [m for m in blocks if m.conv2.weight.requires_grad]
    assert len(trainable) == 13 and G.calls['grad_weight'] == 13        # (layer1 is frozen: frozen_stages=1)
    for m in trainable:
        g = m.conv2.weight.grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def test_detector_simple_test_returns_the_usual_structure(detector):
    from kgdet_amd import grouped_conv as G, synthetic
    cfg, model = detector
    model.eval()
    batch = synthetic.make_batch(1, 'cuda', seed=1, img_shape=IMG, pad_shape=IMG)
    synthetic.calibrate_scores(model, batch, cfg.test_cfg.score_thr)
    G.reset_calls()
    with torch.no_grad():
        res = model.simple_test(batch['img'], batch['img_meta'], rescale=True)
    assert G.calls['bias_act'] == 16 and G.calls['forward'] == 0
    assert isinstance(res, (list, tuple)) and len(res) in (1, 3)
    dets = res[0]          # (per-class boxes[, scores, per-class landmarks]: detector.bbox2result_kp)
    assert len(dets) == cfg.model.bbox_head.num_classes - 1
    assert all(isinstance(d, np.ndarray) and d.ndim == 2 and np.isfinite(d).all() for d in dets)
    assert 0 < sum(len(d) for d in dets) <= cfg.test_cfg.max_per_img
