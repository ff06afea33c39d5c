"""The ResNeXt backbone on the host: registry, state-dict names against the reference's (tests/golden/resnext_golden.npz, made by
tests/golden/make_resnext_golden.py from the reference's module), outputs against its float64 run, the keywords it shares with
ResNet, the envelope of the grouped route and the two config files."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import resnext_cases as X
from tests.dense_refs import ACC_BAR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ('configs/kgdet_moment_x101_32x4d_fpn_1x-demo.py', 'configs/kgdet_moment_x101_32x4d_fpn_1x-deepfashion2.py')


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'resnext_golden.npz'))


def _names_shapes(module):
    sd = module.state_dict()
    return list(sd.keys()), [tuple(t.shape) for t in sd.values()]


def _golden_names_shapes(golden, which):
    names = [str(n) for n in golden['names:' + which]]
    shapes = [tuple(int(v) for v in row if v) for row in golden['shapes:' + which]]
    return names, shapes


def test_registry_builds_resnext_from_a_config_dict():
    from kgdet_amd import backbone
    from kgdet_amd.registry import BACKBONES, build_backbone
    net = build_backbone(dict(type='ResNeXt', style='pytorch', **X.SMALL))
    assert type(net) is backbone.ResNeXt and isinstance(net, backbone.ResNet)
    assert (net.groups, net.base_width) == (8, 4)
    assert net.layer1[0].conv2.groups == 8 and net.layer1[0].conv2.weight.shape == (32, 4, 3, 3)
    assert net.layer2[0].conv2.groups == 8 and net.layer2[0].conv2.weight.shape == (64, 8, 3, 3)
    assert net.layer2[0].conv2.stride == (2, 2) and net.layer2[0].conv3.weight.shape == (512, 64, 1, 1)
    assert 'ResNeXt' in BACKBONES.module_dict and 'ResNet' in BACKBONES.module_dict
    with pytest.raises(KeyError):
        backbone.ResNeXt(depth=18)


@pytest.mark.parametrize('which,kw', [('small', dict(style='pytorch', **X.SMALL)), ('full', X.FULL)])
def test_state_dict_names_and_shapes_are_the_references(golden, which, kw):
    from kgdet_amd.backbone import ResNeXt
    net = ResNeXt(**kw)
    names, shapes = _golden_names_shapes(golden, which)
    got_names, got_shapes = _names_shapes(net)
    assert got_names == names
    assert got_shapes == shapes
    # a checkpoint with the reference's names loads strictly
    sd = {n: (torch.zeros(s, dtype=torch.long) if n.endswith('num_batches_tracked') else torch.full(s, 0.25))
          for n, s in zip(names, shapes)}
    result = net.load_state_dict(sd, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    if which == 'full':
        w = net.layer1[0].conv2
        assert w.groups == 32 and w.weight.shape == (128, 4, 3, 3) and net.layer4[0].conv2.weight.shape == (1024, 32, 3, 3)


def _resnet_names(depth_blocks=(3, 4, 6, 3)):
    """ResNet-50's state dict by rule: stem, then per bottleneck conv<k> / bn<k> and the first block's downsample pair"""
    def bn(prefix):
        return [prefix + '.' + s for s in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')]
    names, shapes = ['conv1.weight'] + bn('bn1'), {}
    inplanes = 64
    shapes['conv1.weight'] = (64, 3, 7, 7)
    for stage, blocks in enumerate(depth_blocks):
        planes = 64 << stage
        for b in range(blocks):
            p = 'layer%d.%d.' % (stage + 1, b)
            for k, shape in ((1, (planes, inplanes, 1, 1)), (2, (planes, planes, 3, 3)), (3, (planes * 4, planes, 1, 1))):
                names += [p + 'conv%d.weight' % k] + bn(p + 'bn%d' % k)
                shapes[p + 'conv%d.weight' % k] = shape
            if b == 0:
                names += [p + 'downsample.0.weight'] + bn(p + 'downsample.1')
                shapes[p + 'downsample.0.weight'] = (planes * 4, inplanes, 1, 1)
            inplanes = planes * 4
    return names, shapes


def test_resnet_keeps_its_module_tree_and_state_dict():
    from kgdet_amd.backbone import Bottleneck, ResNet, ResNeXt
    before = ResNet(depth=50)
    ResNeXt(style='pytorch', **X.SMALL)
    after = ResNet(depth=50)
    names, shapes = _resnet_names()
    for net in (before, after):
        got = net.state_dict()
        assert list(got.keys()) == names
        for n, s in shapes.items():
            assert tuple(got[n].shape) == s
        assert all(type(m) is Bottleneck for layer in (net.layer1, net.layer4) for m in layer)
        assert all(m.groups == 1 for m in net.modules() if isinstance(m, nn.Conv2d))
    assert [n for n, _ in before.named_modules()] == [n for n, _ in after.named_modules()]
    # a ResNeXt of one group is the dense net, name for name and shape for shape
    one = ResNeXt(depth=50, groups=1, base_width=4)
    assert _names_shapes(one) == _names_shapes(before)


def _rel(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize('style', X.STYLES)
def test_outputs_match_the_references_float64_run(golden, style):
    """eval mode (no grad: BatchNorm folded into the convolutions) and train mode (norm_eval, grad on): each output within
    4 x the reference's own float32 error of its float64 output, in max norm relative to the output's max; floor ACC_BAR"""
    from kgdet_amd.backbone import ResNeXt
    net = X.fill(ResNeXt(style=style, **X.SMALL))
    x = X.formula_input(dtype=torch.float32)
    want = [torch.from_numpy(golden['out64:%s:%d' % (style, i)]) for i in range(2)]
    bars = [max(4 * float(golden['err32:%s:%d' % (style, i)]), ACC_BAR) for i in range(2)]
    net.eval()
    with torch.no_grad():
        got = net(x)
    assert len(got) == 2 and [tuple(g.shape) for g in got] == [tuple(w.shape) for w in want]
    for i in range(2):
        r = _rel(got[i], want[i])
        print('%s eval output %d: %.3g (bar %.3g)' % (style, i, r, bars[i]))
        assert r <= bars[i]
    net.train()
    assert not any(m.training for m in net.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm))
    got = net(x.clone().requires_grad_(True))
    assert got[1].requires_grad
    for i in range(2):
        r = _rel(got[i].detach(), want[i])
        print('%s train output %d: %.3g (bar %.3g)' % (style, i, r, bars[i]))
        assert r <= bars[i]


def test_frozen_stages_style_and_zero_init_behave_as_resnets():
    from kgdet_amd.backbone import ResNet, ResNeXt
    kw = dict(depth=50, num_stages=2, strides=(1, 2), dilations=(1, 1), out_indices=(0, 1))
    for frozen in (-1, 0, 1, 2):
        a, b = ResNet(frozen_stages=frozen, **kw), ResNeXt(groups=8, base_width=4, frozen_stages=frozen, **kw)
        a.train(), b.train()
        assert [n for n, p in a.named_parameters() if p.requires_grad] == [n for n, p in b.named_parameters() if p.requires_grad]
        assert [n for n, m in a.named_modules() if m.training] == [n for n, m in b.named_modules() if m.training]
    # style: the stride sits on conv2 ('pytorch') or on conv1 ('caffe')
    p, c = ResNeXt(groups=8, style='pytorch', **kw), ResNeXt(groups=8, style='caffe', **kw)
    assert (p.layer2[0].conv1.stride, p.layer2[0].conv2.stride) == ((1, 1), (2, 2))
    assert (c.layer2[0].conv1.stride, c.layer2[0].conv2.stride) == ((2, 2), (1, 1))
    assert p.layer2[1].conv2.stride == c.layer2[1].conv2.stride == (1, 1)
    # zero_init_residual: the last BatchNorm of every block starts at zero (or at one)
    for zero in (True, False):
        n = ResNeXt(groups=8, zero_init_residual=zero, **kw)
        n.init_weights()
        for m in n.modules():
            if hasattr(m, 'norm3'):
                assert float(m.norm3.weight.detach().abs().max()) == (0.0 if zero else 1.0)
                assert float(m.norm2.weight.detach().min()) == 1.0
    # norm_eval=False: BatchNorms of the unfrozen stages train
    n = ResNeXt(groups=8, norm_eval=False, frozen_stages=1, **kw)
    n.train()
    assert n.layer2[0].bn2.training and not n.layer1[0].bn2.training


def test_deformable_conv2_takes_the_groups_of_the_dcn_dict():
    from kgdet_amd.backbone import ResNet, ResNeXt
    kw = dict(depth=50, num_stages=2, strides=(1, 2), dilations=(1, 1), out_indices=(0, 1),
              dcn=dict(modulated=False, groups=8, deformable_groups=1, fallback_on_stride=False), stage_with_dcn=(False, True))
    n = ResNeXt(groups=8, base_width=4, **kw)
    assert n.layer1[0].conv2.groups == 8 and type(n.layer1[0].conv2) is nn.Conv2d
    assert n.layer2[0].conv2.groups == 8 and n.layer2[0].conv2.weight.shape == (64, 8, 3, 3)
    assert n.layer2[0].conv2_offset.weight.shape == (18, 64, 3, 3)
    assert ResNet(**kw).layer2[0].conv2.groups == 1          # (the dense block never read dcn['groups'])


def test_grouped_route_envelope():
    from kgdet_amd import grouped_conv as G
    ok = dict(stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=3)
    assert G.shape_ok((2, 12, 5, 7), (12, 4, 3, 3), **ok)
    assert G.shape_ok((2, 96, 5, 7), (96, 32, 3, 3), **dict(ok, stride=(2, 2)))
    assert G.shape_ok((1, 8, 1, 1), (8, 8, 3, 3), **dict(ok, groups=1))
    for x_shape, w_shape, over in [
            ((2, 12, 5, 7), (12, 4, 3, 3), dict(stride=(1, 2))), ((2, 12, 5, 7), (12, 4, 3, 3), dict(stride=(3, 3))),
            ((2, 12, 5, 7), (12, 4, 3, 3), dict(padding=(0, 0))), ((2, 12, 5, 7), (12, 4, 3, 3), dict(dilation=(2, 2))),
            ((2, 12, 5, 7), (12, 4, 3, 3), dict(groups=4)), ((2, 12, 5, 7), (12, 4, 1, 1), {}),
            ((2, 12, 5, 7), (12, 4, 5, 5), {}), ((2, 15, 5, 7), (15, 5, 3, 3), {}), ((2, 6, 5, 7), (6, 2, 3, 3), {}),
            ((2, 192, 5, 7), (192, 64, 3, 3), {}), ((2, 16, 5, 7), (12, 4, 3, 3), {}), ((0, 12, 5, 7), (12, 4, 3, 3), {}),
            ((2, 12, 0, 7), (12, 4, 3, 3), {}), ((12, 5, 7), (12, 4, 3, 3), {}), ((70000, 12, 5, 7), (12, 4, 3, 3), {})]:
        assert not G.shape_ok(x_shape, w_shape, **dict(ok, **over)), (x_shape, w_shape, over)
    # CPU tensors never take the route, whatever their shape
    x, w = torch.zeros(2, 12, 5, 7), torch.zeros(12, 4, 3, 3)
    assert not G.applicable(x, w, **ok)
    assert not G.applicable(x.double(), w.double(), **ok)
    assert set(G.calls) == {'forward', 'bias_act', 'grad_input', 'grad_weight'}


def test_builder_and_config_files_build_the_detector():
    from kgdet_amd import backbone, configs, numerics
    from kgdet_amd.registry import Config, build_detector
    base, r50 = configs.kgdet_x101_fpn(), configs.kgdet_r50_fpn()
    assert base.model.backbone == dict(type='ResNeXt', depth=101, groups=32, base_width=4, num_stages=4,
                                       out_indices=(0, 1, 2, 3), frozen_stages=1, style='pytorch')
    assert {k: v for k, v in base.model.items() if k not in ('backbone', 'pretrained')} == \
        {k: v for k, v in r50.model.items() if k not in ('backbone', 'pretrained')}
    assert (base.train_cfg, base.test_cfg) == (r50.train_cfg, r50.test_cfg)
    assert configs.kgdet_x101_fpn(groups=64).model.pretrained.endswith('resnext101_64x4d')
    for rel in CONFIGS:
        cfg = Config.fromfile(os.path.join(ROOT, rel))
        assert cfg.model.backbone == base.model.backbone
        assert cfg.model.bbox_head == base.model.bbox_head and cfg.model.neck == base.model.neck
        assert cfg.model.pretrained == (None if rel.endswith('demo.py') else base.model.pretrained)
        for key in ('data', 'optimizer', 'optimizer_config', 'lr_config', 'total_epochs', 'work_dir'):
            assert key in cfg
        assert cfg.data.test.test_mode and cfg.data.train.type == 'DeepFashion2Dataset'
    small = configs.kgdet_x101_fpn(depth=50)
    model = build_detector(small.model, train_cfg=small.train_cfg, test_cfg=small.test_cfg)
    assert type(model.backbone) is backbone.ResNeXt and model.backbone.layer3[0].conv2.groups == 32
    # the envelope guard enumerates the model; the grouped weights are not rows of its table
    layers = numerics.EnvelopeGuard(model).layers
    grouped = {id(m) for m in model.modules() if isinstance(m, nn.Conv2d) and m.groups > 1}
    assert len(grouped) == 16 and layers and not any(id(l.conv) in grouped for l in layers)
    cfg = Config.fromfile(os.path.join(ROOT, CONFIGS[0]))
    full = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    assert sum(1 for m in full.modules() if isinstance(m, nn.Conv2d) and m.groups == 32) == 33
