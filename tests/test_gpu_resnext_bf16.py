"""The ResNeXt backbone at bf16 autocast inference with the grouped conv2 on csrc/grouped_conv_nhwc.hip (grouped_conv.BF16):
the small net of tests/resnext_cases.py (4 and 8 channels per group) with conv2 taking its shift and ReLU in the store, and with
conv2 raw in front of the fused conv3 kernel; single grouped convolutions of 16 and 32 channels per group through
``backbone._conv_bn``; the switch off; the ``1`` setting; one detection pass of a KGDet detector on a ResNeXt-50 32x4d.

Bars: against the fp32 features the route stays finite, within the project's BF16_BAR of their max, and within 2 x the
switch-off route's own error measured in the same test -- both routes round alike per layer and differ in the fp32 accumulation
order only, while a dropped tap or a wrong group is off by the scale of the features."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import resnext_cases as X

pytestmark = pytest.mark.gpu

INPUT = (2, 3, 64, 96)
GROUPED = 7          # grouped conv2 of the small net: 3 in layer1 (4 channels per group), 4 in layer2 (8; the first at stride 2)
IMG = (160, 192, 3)
BF16_BAR = 0.05      # of the fp32 features' max: the bar of test_gpu_backbone's bf16 inference comparison


@pytest.fixture(autouse=True)
def forced_route(monkeypatch):
    from kgdet_amd import backbone, conv1x1, grouped_conv
    monkeypatch.setattr(grouped_conv, 'BF16', 'force')
    monkeypatch.setattr(grouped_conv, 'ENABLED', True)
    conv1x1._entries.clear(), conv1x1._fold_entries.clear()
    backbone.clear_fold_cache()
    yield
    conv1x1._entries.clear(), conv1x1._fold_entries.clear()
    backbone.clear_fold_cache()


def _small():
    from kgdet_amd.backbone import ResNeXt
    net = X.fill(ResNeXt(style='pytorch', **X.SMALL)).cuda()
    net.eval()
    return net


def _bf16(net, x, calls=3):
    """the features under bf16 autocast (the measured 1x1 route choices settle in the first calls) and the launches of the LAST
    call: (outputs, calls_nhwc, calls)"""
    from kgdet_amd import grouped_conv as G
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        for _ in range(calls - 1):
            net(x)
        G.reset_calls(), G.reset_calls_nhwc()
        out = net(x)
    return out, dict(G.calls_nhwc), dict(G.calls)


def _hold(tag, new, old, want):
    scale = float(want.abs().max())
    e_new, e_old = float((new.float() - want).abs().max()), float((old.float() - want).abs().max())
    print('%s: route %.4g, switch off %.4g of the fp32 max (%.3f of 2 x)' % (tag, e_new / scale, e_old / scale, e_new / max(2 * e_old, 1e-30)))
    assert bool(torch.isfinite(new.float()).all()), tag
    assert e_new <= BF16_BAR * scale, tag
    assert e_new <= 2 * e_old, tag


@pytest.mark.parametrize('raw', [False, True], ids=['bias_act', 'raw'])
def test_small_net_on_the_route_against_fp32_and_the_switch_off(raw, monkeypatch):
    from kgdet_amd import backbone, grouped_conv as G
    if raw:     # every conv2 hands its raw output and its shift to conv3
        monkeypatch.setattr(backbone, 'fused_residual_ready', lambda conv3, B, H, W: True)
    else:       # every conv2 takes its shift and its ReLU in the store
        monkeypatch.setattr(backbone, 'RAW_BRANCHES', False)
    net = _small()
    x = X.formula_input(INPUT, torch.float32).cuda()
    with torch.no_grad():
        want = net(x)
    new, nhwc, fp32 = _bf16(net, x)
    assert nhwc == (dict(raw=GROUPED, bias_act=0) if raw else dict(raw=0, bias_act=GROUPED))
    assert not any(fp32.values())
    monkeypatch.setattr(G, 'BF16', '0')
    old, nhwc, fp32 = _bf16(net, x)
    assert not any(nhwc.values()) and not any(fp32.values())
    for i in range(2):
        assert new[i].shape == want[i].shape and new[i].dtype == old[i].dtype
        _hold('%s output %d' % ('raw' if raw else 'bias_act', i), new[i], old[i], want[i])


def _pair(C, groups, stride):
    conv = nn.Conv2d(C, C, 3, stride, 1, groups=groups, bias=False)
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        conv.weight.copy_(X.formula('conv2.weight', tuple(conv.weight.shape)).float())
        for name in ('weight', 'bias', 'running_mean', 'running_var'):
            getattr(bn, name).copy_(X.formula('bn2.' + name, (C,)).float())
    return conv.cuda().eval(), bn.cuda().eval()


@pytest.mark.parametrize('cpg,groups,stride', [(16, 3, 1), (16, 5, 2), (32, 3, 1), (32, 2, 2), (8, 9, 2), (4, 2, 1)])
def test_single_convolutions_through_conv_bn(cpg, groups, stride, monkeypatch):
    """16 and 32 channels per group (the small net has 4 and 8), shift + ReLU in the store and raw; with the switch off the same
    call returns the bits of F.conv2d + the epilogue pass on the cached folded weight: the route before this switch existed"""
    from kgdet_amd import backbone, grouped_conv as G
    C = cpg * groups
    conv, bn = _pair(C, groups, stride)
    x = X.formula_input((2, C, 19, 37), torch.float32).cuda()
    x16 = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        want = F.relu(bn(conv(x16.float())))
        with torch.autocast('cuda', dtype=torch.bfloat16):
            G.reset_calls(), G.reset_calls_nhwc()
            new = backbone._conv_bn(conv, bn, x16, relu=True)
            new_raw, shift = backbone._conv_bn(conv, bn, x16, relu=True, raw=True)
            assert G.calls_nhwc == dict(raw=1, bias_act=1) and not any(G.calls.values())
            monkeypatch.setattr(G, 'BF16', '0')
            G.reset_calls_nhwc()
            old = backbone._conv_bn(conv, bn, x16, relu=True)
            old_raw, shift_old = backbone._conv_bn(conv, bn, x16, relu=True, raw=True)
            assert not any(G.calls_nhwc.values()) and not any(G.calls.values())
            hit = backbone._fold_cache[(id(conv), True)]
            parent_raw = F.conv2d(x16, hit.weight, None, conv.stride, conv.padding, conv.dilation, conv.groups)
            parent = backbone._epilogue_(parent_raw.clone(), hit.bias, None, True)
    assert torch.equal(old.view(torch.int16), parent.view(torch.int16))
    assert torch.equal(old_raw.view(torch.int16), parent_raw.view(torch.int16)) and shift is shift_old is hit.bias
    for t in (new, new_raw):
        assert t.dtype == torch.bfloat16 and t.shape == want.shape and t.is_contiguous(memory_format=torch.channels_last)
    _hold('cpg %d stride %d shift + ReLU' % (cpg, stride), new, old, want)
    raw_want = F.conv2d(x16.float(), hit.weight.float(), None, conv.stride, conv.padding, conv.dilation, conv.groups)
    _hold('cpg %d stride %d raw' % (cpg, stride), new_raw, old_raw, raw_want)


def _expected(net, classes):
    convs = [m.conv2 for m in net.modules() if hasattr(m, 'conv2')]
    return sum(1 for c in convs if (c.weight.shape[1], c.stride[0]) not in classes)


def test_setting_1_skips_exactly_the_torch_classes(monkeypatch):
    from kgdet_amd import backbone, grouped_conv as G
    monkeypatch.setattr(backbone, 'RAW_BRANCHES', False)
    net = _small()
    x = X.formula_input(INPUT, torch.float32).cuda()
    monkeypatch.setattr(G, 'BF16', '1')
    # the classes as they are measured, then one class of the small net: the stride-2 conv2 at the head of layer2
    _, nhwc, _ = _bf16(net, x)
    assert nhwc == dict(raw=0, bias_act=_expected(net, G.TORCH_CLASSES_BF16))
    for classes, want in ((frozenset([(8, 2)]), GROUPED - 1), (frozenset([(4, 1), (16, 1)]), GROUPED - 3),
                          (frozenset([(4, 2), (32, 1)]), GROUPED)):
        monkeypatch.setattr(G, 'TORCH_CLASSES_BF16', classes)
        assert _expected(net, classes) == want
        _, nhwc, _ = _bf16(net, x, calls=1)
        assert nhwc == dict(raw=0, bias_act=want)
    monkeypatch.setattr(G, 'BF16', 'force')
    _, nhwc, _ = _bf16(net, x, calls=1)
    assert nhwc == dict(raw=0, bias_act=GROUPED)


def test_switch_off_equals_the_route_without_grouped_kernels(monkeypatch):
    """BF16 = '0' (the default): no launch, and the bits of a run with every grouped kernel off (ENABLED = False)"""
    from kgdet_amd import grouped_conv as G
    net = _small()
    x = X.formula_input(INPUT, torch.float32).cuda()
    monkeypatch.setattr(G, 'BF16', '0')
    off, nhwc, fp32 = _bf16(net, x)
    assert not any(nhwc.values()) and not any(fp32.values())
    monkeypatch.setattr(G, 'ENABLED', False)
    monkeypatch.setattr(G, 'BF16', 'force')          # (KGDET_GROUPED_CONV=0 turns the bf16 route off as well)
    torch_only, nhwc, fp32 = _bf16(net, x, calls=1)
    assert not any(nhwc.values()) and not any(fp32.values())
    for a, b in zip(off, torch_only):
        assert a.dtype == b.dtype and torch.equal(a.float(), b.float())


def test_detector_simple_test_on_the_route():
    from kgdet_amd import configs, grouped_conv as G, synthetic
    from kgdet_amd.registry import build_detector
    cfg = configs.kgdet_x101_fpn(depth=50)
    torch.manual_seed(0)
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda()
    model.eval()
    batch = synthetic.make_batch(1, 'cuda', seed=1, img_shape=IMG, pad_shape=IMG)
    synthetic.calibrate_scores(model, batch, cfg.test_cfg.score_thr, autocast=torch.autocast('cuda', dtype=torch.bfloat16))
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        model.simple_test(batch['img'], batch['img_meta'], rescale=True)      # (the measured route choices settle)
        G.reset_calls(), G.reset_calls_nhwc()
        res = model.simple_test(batch['img'], batch['img_meta'], rescale=True)
    assert sum(G.calls_nhwc.values()) == 16 and not any(G.calls.values())
    assert isinstance(res, (list, tuple)) and len(res) in (1, 3)
    dets = res[0]
    assert len(dets) == cfg.model.bbox_head.num_classes - 1
    assert all(isinstance(d, np.ndarray) and d.ndim == 2 and np.isfinite(d).all() for d in dets)
    assert 0 < sum(len(d) for d in dets) <= cfg.test_cfg.max_per_img
