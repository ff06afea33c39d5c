"""The envelope guard of the fp16-part dense convolutions end to end (kgdet_amd/numerics.py, conv1x1.set_bf16_parts, the callers
in checkpoint.py and runner.py) on the GPU.

(a) a conv(64 -> 64, k = 1 / 3) + frozen BatchNorm whose channel 7 has running_var = 1e-12 (s = 316, |w s| far beyond 255.875):
    under the policy `bf16` every channel -- 7 included -- is within 2e-5 of ITS OWN output scale of F.conv2d + BatchNorm in
    float64 (the bar of test_step_scope_packs_follow_weight_updates for bf16-part convolutions, applied per channel: channel 7's
    outputs are 300 times the others', a whole-tensor scale would let the others pass with any error), through the folded
    inference route and through the training _ConvBNActFold node; the gradients within that test's 5e-5.  `raise` names the
    layer; `off` is the arithmetic from before the guard: bit-equal, in EVERY channel, to an explicit format-1 pack of the same
    folded weight applied directly (the kernels as no route can touch them -- this stands in for "a run without the module"),
    with channel 7 off by more than 1e-2.
(b) a model inside the envelope: no violations, nothing rerouted, outputs bit-equal with the guard on and `off`.
(c) numerics.audit: an input whose channel 3 is scaled by 1e5 is reported with numpy's counts beyond 65504 and 131008.
(d) a reroute underneath a captured GraphedTrainStep raises when called directly and is re-captured by the Runner's epoch-end
    check (the model and batch of tests/test_gpu_runner.py)."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from kgdet_amd import backbone, conv1x1, numerics
from kgdet_amd import runner as rn

pytestmark = pytest.mark.gpu


class _Pair(nn.Module):
    def __init__(self, k):
        super().__init__()
        self.conv1 = nn.Conv2d(64, 64, k, padding=k // 2, bias=False)
        self.bn1 = nn.BatchNorm2d(64)

    def forward(self, x):
        return backbone.conv_bn(self.conv1, self.bn1, x)


def _pair(k, tiny, seed=0):
    g = torch.Generator().manual_seed(1000 * k + seed)
    m = _Pair(k)
    with torch.no_grad():
        m.conv1.weight.copy_(torch.randn(64, 64, k, k, generator=g))
        m.bn1.running_var.copy_(torch.rand(64, generator=g) * 1.5 + 0.5)
        m.bn1.running_mean.copy_(torch.randn(64, generator=g) * 0.1)
        m.bn1.bias.copy_(torch.randn(64, generator=g) * 0.1)        # gamma stays 1
        if tiny:
            m.bn1.running_var[7] = 1e-12
    x = torch.randn(2, 64, 12, 16, generator=g)
    return m.cuda().eval(), x.cuda()


def _folded_max(m):
    s = (m.bn1.weight.detach().double() / torch.sqrt(m.bn1.running_var.double() + m.bn1.eps)).view(-1, 1)
    return (m.conv1.weight.detach().double().flatten(1) * s).abs().max(1).values.cpu().numpy()


def _reference(m, x, gy=None):
    """F.conv2d + BatchNorm (eval) in float64 on the CPU -> y [, grad_x, grad_w for the cotangent gy]"""
    w = m.conv1.weight.detach().double().cpu().requires_grad_(True)
    xd = x.detach().double().cpu().requires_grad_(True)
    bn = m.bn1
    y = F.batch_norm(F.conv2d(xd, w, padding=w.shape[2] // 2), bn.running_mean.double().cpu(), bn.running_var.double().cpu(),
                     bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu(), False, 0.0, bn.eps)
    if gy is None:
        return y.detach()
    gx, gw = torch.autograd.grad(y, [xd, w], gy.double().cpu())
    return y.detach(), gx, gw


def _channel_errors(y, ref):
    """per output channel: max |y - ref| over that channel's max |ref|"""
    d = (y.detach().double().cpu() - ref).abs().amax((0, 2, 3))
    return (d / ref.abs().amax((0, 2, 3))).numpy()


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    monkeypatch.delenv('KGDET_ENVELOPE', raising=False)
    yield
    conv1x1._bf16_parts.clear()
    conv1x1._table = None
    backbone.clear_fold_cache()


@pytest.mark.parametrize('k', [1, 3])
def test_tiny_variance_channel_inference(k, monkeypatch):
    m, x = _pair(k, tiny=True)
    fm = _folded_max(m)
    assert fm[7] > numerics.WEIGHT_LIMIT and np.delete(fm, 7).max() < numerics.WEIGHT_LIMIT       # the inputs are what they claim
    ref = _reference(m, x)

    # off: today's arithmetic, byte for byte -- and channel 7 is wrong
    monkeypatch.setenv('KGDET_ENVELOPE', 'off')
    assert numerics.enforce(m) == ([], [])
    with torch.no_grad():
        y_off = m(x)
        scale = m.bn1.weight * torch.rsqrt(m.bn1.running_var + m.bn1.eps)
        w = (m.conv1.weight * scale.view(-1, 1, 1, 1)).detach().contiguous()
        shift = (m.bn1.bias - m.bn1.running_mean * scale).detach().float().contiguous()
        y_before = conv1x1._apply(conv1x1._pack(w, False, f16=True), x, 64, k * k, 1, shift, None, False)
    assert torch.equal(y_off, y_before)
    e = _channel_errors(y_off, ref)
    print('k=%d off: channel 7 %.3e, others max %.3e' % (k, e[7], np.delete(e, 7).max()))
    assert e[7] > 1e-2 and np.delete(e, 7).max() <= 2e-5

    # raise: names the layer
    monkeypatch.setenv('KGDET_ENVELOPE', 'raise')
    with pytest.raises(numerics.EnvelopeError, match=r'conv1 \(folded\)'):
        numerics.enforce(m)

    # bf16: rerouted (the folded copy packed under `off` is dropped with the route), every channel right
    monkeypatch.setenv('KGDET_ENVELOPE', 'bf16')
    violations = numerics.guard_for(m).check()
    assert [v.name for v in violations] == ['conv1 (folded)'] and violations[0].limit == 'clamp'
    with pytest.warns(RuntimeWarning, match='bf16 parts'):
        rerouted = numerics.apply_policy(violations)
    assert len(rerouted) == 1 and conv1x1.bf16_parts(m.conv1.weight)
    with torch.no_grad():
        y = m(x)
    hit = backbone._fold_cache[(id(m.conv1), False)]
    assert hit.packed is not None and hit.packed.kgdet_f16 is False
    e = _channel_errors(y, ref)
    print('k=%d bf16: channel 7 %.3e, others max %.3e' % (k, e[7], np.delete(e, 7).max()))
    assert e.max() <= 2e-5, e


@pytest.mark.parametrize('k', [1, 3])
def test_tiny_variance_channel_training_fold_node(k):
    m, x = _pair(k, tiny=True)
    x.requires_grad_(True)
    gy = torch.randn(2, 64, 12, 16, generator=torch.Generator().manual_seed(5)).cuda()
    gy[:, 7] /= 316.0                              # (so that channel 7 does not drown the other channels' share of grad_x)
    ref, gx_ref, gw_ref = _reference(m, x, gy)
    with conv1x1.step_scope():                     # first scope: the pair joins the folded set (its images marked fp16)
        m(x)
    e0 = conv1x1._fold_entries[id(m.conv1.weight)]
    assert e0.img.kgdet_f16 is conv1x1.FORWARD_F16
    with pytest.warns(RuntimeWarning, match='bf16 parts'):
        violations, rerouted = numerics.enforce(m)      # default policy: bf16
    assert [v.name for v in rerouted] == ['conv1 (folded)'] and e0.img.kgdet_f16 is False and conv1x1._table is None
    with conv1x1.step_scope():                     # second scope: packed again, in bf16 parts, by the scope's launch
        y = m(x)
        assert 'ConvBNActFold' in type(y.grad_fn).__name__
    gx, gw = torch.autograd.grad(y, [x, m.conv1.weight], gy)
    e = _channel_errors(y, ref)
    egx = float((gx.double().cpu() - gx_ref).abs().max() / gx_ref.abs().max())
    egw = float((gw.double().cpu() - gw_ref).abs().max() / gw_ref.abs().max())
    print('k=%d fold node: forward channel 7 %.3e, others max %.3e, grad_x %.3e, grad_w %.3e' % (k, e[7], np.delete(e, 7).max(),
                                                                                               egx, egw))
    assert e.max() <= 2e-5, e
    assert egx <= 5e-5 and egw <= 5e-5


@pytest.mark.parametrize('k', [1, 3])
def test_model_inside_the_envelope_is_left_alone(k, monkeypatch):
    m, x = _pair(k, tiny=False)
    assert _folded_max(m).max() < numerics.WEIGHT_LIMIT
    with torch.no_grad():
        monkeypatch.setenv('KGDET_ENVELOPE', 'off')
        assert numerics.enforce(m) == ([], [])
        y_off = m(x)
        backbone.clear_fold_cache()
        monkeypatch.setenv('KGDET_ENVELOPE', 'bf16')
        guard = numerics.guard_for(m)
        assert guard.check() == [] and numerics.enforce(m) == ([], [])
        assert not conv1x1._bf16_parts
        y_on = m(x)
    assert torch.equal(y_on, y_off)
    assert [l.name for l in guard.layers] == ['conv1 (folded)', 'conv1']
    # the wrapper against numpy on the model's own tensors: one launch, one structured array
    rec = numerics.scan([m.conv1.weight.detach()], [numerics.Scale(m.bn1.weight.detach(), m.bn1.running_var, m.bn1.eps, 64 * k * k)])
    assert rec.dtype == numerics.RECORD and rec.shape == (1,)
    assert abs(float(rec['max'][0]) - _folded_max(m).max()) <= 1e-5 * _folded_max(m).max() and rec['over1'][0] == 0


def test_audit_counts_the_activations_beyond_the_limits():
    m, x = _pair(3, tiny=False)
    model = nn.Sequential(m).eval()
    x = x.clone()
    x[:, 3] *= 1e5
    patched = conv1x1._apply
    rows = numerics.audit(model, x)
    assert conv1x1._apply is patched
    a = np.abs(x.cpu().numpy())
    assert len(rows) == 1 and rows[0]['name'] == '0#1' and rows[0]['shape'] == ((2, 64, 12, 16), 64, 9)
    assert rows[0]['over_limit'] == int((a > np.float32(65504.0)).sum()) > 0
    assert rows[0]['over_clamp'] == int((a > np.float32(131008.0)).sum()) > 0
    assert rows[0]['over_limit'] > rows[0]['over_clamp'] and rows[0]['nonfinite'] == 0
    assert np.float32(rows[0]['max']) == a.max()
    quiet = numerics.audit(model, torch.randn_like(x))
    assert quiet[0]['over_limit'] == 0 and quiet[0]['over_clamp'] == 0


def test_load_checkpoint_applies_the_policy(tmp_path, monkeypatch):
    from kgdet_amd import checkpoint
    src, _ = _pair(1, tiny=True)
    checkpoint.save_checkpoint(src, str(tmp_path / 'tiny.pth'))
    monkeypatch.setenv('KGDET_ENVELOPE', 'raise')
    dst, _ = _pair(1, tiny=False, seed=1)
    with pytest.raises(numerics.EnvelopeError, match=r'conv1 \(folded\)'):
        checkpoint.load_checkpoint(dst, str(tmp_path / 'tiny.pth'))
    monkeypatch.setenv('KGDET_ENVELOPE', 'bf16')
    dst, _ = _pair(1, tiny=False, seed=1)
    with pytest.warns(RuntimeWarning, match='bf16 parts'):
        checkpoint.load_checkpoint(dst, str(tmp_path / 'tiny.pth'))
    assert conv1x1.bf16_parts(dst.conv1.weight)


def test_reroute_under_a_captured_step_raises_and_the_runner_recaptures():
    from tests.test_gpu_runner import _graph_case
    make, batch = _graph_case('kgdet')
    model, opt, hook = make()
    g = rn.GraphedTrainStep(model, opt, hook, batch, warmup=2)
    g.step()
    torch.cuda.synchronize()
    block = model.backbone.layer2[1]
    w = block.conv1.weight
    with torch.no_grad():
        block.bn1.running_var[7] = 1e-12
        w[7] *= 30.0 / float(w[7].abs().max()) * 0.044          # row 7: max |w| = 1.32, |w s| = 417 > 255.875
    with pytest.raises(numerics.EnvelopeError, match='build the graphed step again'):
        conv1x1.set_bf16_parts(w)
    assert not conv1x1.bf16_parts(w) and g.graph is not None
    runner = rn.Runner(model, opt, logger=lambda s: None)
    runner.attach_graphed(g)
    with pytest.warns(RuntimeWarning, match='bf16 parts'):
        rerouted = runner.check_envelope()
    assert [v.name for v in rerouted] == ['backbone.layer2.1.conv1 (folded)']
    assert conv1x1.bf16_parts(w) and g.graph is None and runner.graphed is not g and runner.graphed.graph is not None
    assert runner.graphed.steps == g.steps == 1
    e = conv1x1._fold_entries[id(w)]
    assert e.img.kgdet_f16 is False
    out = runner.graphed.step()
    torch.cuda.synchronize()
    assert torch.isfinite(out['loss']).item()
    assert runner.check_envelope() == []            # still outside, already routed: the step is left alone
    assert runner.graphed.graph is not None


# ------------------------------------------------------------------------------------- a bottleneck with a deformable conv2
def _dcn_block(stride, tiny):
    """backbone.Bottleneck(64 -> 128, conv2 deformable) with frozen statistics; ``tiny``: channel 7 of norm3 and channel 5 of
    the downsample BatchNorm have running_var = 1e-12"""
    torch.manual_seed(11)
    down = nn.Sequential(nn.Conv2d(64, 128, 1, stride=stride, bias=False), nn.BatchNorm2d(128))
    blk = backbone.Bottleneck(64, 32, stride=stride, downsample=down,
                              dcn=dict(modulated=False, deformable_groups=1, fallback_on_stride=False))
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
        blk.conv2_offset.weight.normal_(0, 0.05)
        blk.conv3.weight.normal_(0, 1.0)                 # (|w| up to ~4, as in _pair: x 316 beyond the clamp, x 1.4 far inside)
        blk.downsample[0].weight.normal_(0, 1.0)
        if tiny:
            blk.norm3.running_var[7] = 1e-12
            blk.downsample[1].running_var[5] = 1e-12
            # (eight weights of 4 in each of the two rows: |w s| = 1265, beyond the clamp at 511.75 whatever the draw gave)
            blk.conv3.weight[7, :8, 0, 0] = torch.tensor([4., -4., 4., 4., -4., 4., -4., 4.])
            blk.downsample[0].weight[5, :8, 0, 0] = torch.tensor([4., 4., -4., 4., -4., -4., 4., 4.])
    return blk.cuda().eval(), torch.randn(2, 64, 12, 16).cuda()


def _dcn_block_reference(blk, x, stride):
    """the block in float64 on the CPU, conv2 as the grid_sample formulation of tests/torch_ref.py"""
    import copy
    from tests import torch_ref
    ref = copy.deepcopy(blk).double().cpu()
    with torch.no_grad():
        xd = x.double().cpu()
        out = ref.relu(ref.norm1(ref.conv1(xd)))
        out = torch_ref.deform_conv(out, ref.conv2_offset(out), ref.conv2.weight, stride=stride, padding=1, dilation=1)
        out = ref.norm3(ref.conv3(ref.relu(ref.norm2(out))))
        return ref.relu(out + ref.downsample(xd))


def _block_errors(y, ref):
    """_channel_errors with a floor under a channel's scale: a channel the final ReLU leaves (almost) dead is held to 1e-3 of the
    median channel's scale instead of to its own"""
    scale = ref.abs().amax((0, 2, 3))
    d = (y.detach().double().cpu() - ref).abs().amax((0, 2, 3))
    return (d / scale.clamp_min(1e-3 * float(scale.median()))).numpy()


@pytest.mark.parametrize('stride', [1, 2])
def test_bottleneck_with_deformable_conv2_is_scanned_and_rerouted(stride, monkeypatch):
    """conv3 and the downsample branch of a bottleneck with a deformable conv2 run through backbone.conv_bn like the dense
    block's, so the guard lists them (conv2 and conv2_offset, which never take the fp16-part route, stay out): with a tiny
    variance in norm3 (channel 7) and in the downsample BatchNorm (channel 5) `off` leaves channel 7 of the block's inference
    output wrong by more than 1e-2 of its own scale, `raise` names the layers, and under `bf16` both weights are rerouted and
    every channel is within 1e-4 of its own scale of the float64 block (the bar of
    test_bottleneck_dcn_option_matches_torch_reference, applied per channel) -- in inference and through the training nodes
    (autograd on, frozen statistics; the strided downsample takes the fp16-part route only there)."""
    blk, x = _dcn_block(stride, tiny=True)
    ref = _dcn_block_reference(blk, x, stride)
    names = [l.name for l in numerics.guard_for(blk).layers]
    assert names == ['conv1 (folded)', 'conv3 (folded)', 'downsample.0 (folded)', 'conv1', 'conv3', 'downsample.0'], names

    monkeypatch.setenv('KGDET_ENVELOPE', 'off')
    assert numerics.enforce(blk) == ([], [])
    with torch.no_grad():
        e = _block_errors(blk(x), ref)
    print('dcn block stride %d off: channel 7 %.3e, channel 5 %.3e, others max %.3e' % (stride, e[7], e[5], np.delete(e, [5, 7]).max()))
    assert e[7] > 1e-2 and np.delete(e, [5, 7]).max() <= 1e-4

    monkeypatch.setenv('KGDET_ENVELOPE', 'raise')
    with pytest.raises(numerics.EnvelopeError, match=r'conv3 \(folded\)'):
        numerics.enforce(blk)

    monkeypatch.setenv('KGDET_ENVELOPE', 'bf16')
    violations = numerics.guard_for(blk).check()
    assert [v.name for v in violations] == ['conv3 (folded)', 'downsample.0 (folded)']
    with pytest.warns(RuntimeWarning, match='bf16 parts'):
        rerouted = numerics.apply_policy(violations)
    assert len(rerouted) == 2 and conv1x1.bf16_parts(blk.conv3.weight) and conv1x1.bf16_parts(blk.downsample[0].weight)
    with torch.no_grad():
        e = _block_errors(blk(x), ref)
    print('dcn block stride %d bf16 inference: channel 7 %.3e, channel 5 %.3e, max %.3e' % (stride, e[7], e[5], e.max()))
    assert e.max() <= 1e-4, e
    xg = x.clone().requires_grad_(True)
    for _ in range(2):              # (the second scope runs the folded nodes)
        with conv1x1.step_scope():
            y = blk(xg)
        e = _block_errors(y, ref)
        print('dcn block stride %d bf16 training node: channel 7 %.3e, channel 5 %.3e, max %.3e' % (stride, e[7], e[5], e.max()))
        assert e.max() <= 1e-4, e


def test_bottleneck_with_deformable_conv2_inside_the_envelope_is_left_alone():
    blk, x = _dcn_block(2, tiny=False)
    assert numerics.guard_for(blk).check() == [] and numerics.enforce(blk) == ([], [])
    assert not conv1x1._bf16_parts
    with torch.no_grad():
        assert _block_errors(blk(x), _dcn_block_reference(blk, x, 2)).max() <= 1e-4
