"""CPU: the numpy restatement of the range-scan record (tests/envelope_refs.py) on hand-computed cases, and the host logic of
kgdet_amd/numerics.py + conv1x1.set_bf16_parts against a FAKE scan (the reference, injected in place of the device table): layer
enumeration, table rebuilds, the four policies, re-marking, and `off` never touching the library."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

from kgdet_amd import conv1x1, numerics
from tests import envelope_refs as ref


# ---- the reference itself ----------------------------------------------------------------------------------------------------
def test_record_counts_and_max_by_hand():
    v = np.array([0.0, -3.0, 2.0, np.inf, -np.inf, np.nan, 255.875, -256.0], np.float32)
    mx, bad, o1, o2 = ref.record(v, 255.875, 300.0)
    assert (mx, bad, o1, o2) == (np.float32(256.0), 3, 3, 2)       # inf counts beyond both limits, NaN beyond neither
    assert ref.record(np.zeros(5, np.float32), 1.0, 2.0) == (np.float32(0), 0, 0, 0)
    assert ref.record(np.array([np.nan], np.float32), 1.0, 2.0) == (np.float32(0), 1, 0, 0)


def test_record_limit_is_strict_and_scale_is_float32():
    hi = np.float32(255.875)
    assert ref.record(np.array([hi, np.nextafter(hi, np.float32(np.inf))], np.float32), hi, hi)[2:] == (1, 1)
    assert ref.record(np.array([hi], np.float32), hi, hi)[2:] == (0, 0)
    var, eps = np.array([1e-12, 1.0], np.float32), 1e-5
    s = ref.row_scale(var, eps)
    assert s.dtype == np.float32
    assert s[0] == np.float32(1) / np.sqrt(np.float32(np.float32(1e-12) + np.float32(1e-5)))
    p = ref.products(np.array([1.0, 2.0, 3.0, 4.0], np.float32), inner=2, var=var, eps=eps)
    assert p.dtype == np.float32 and p[1] == np.float32(2.0) * s[0] and p[2] == np.float32(3.0) * s[1]
    assert ref.ulps(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1
    assert ref.margin(np.array([255.875 * (1 + 2.0 ** -10)]), 255.875) == pytest.approx(2.0 ** -10)


# ---- host logic against a fake scan ------------------------------------------------------------------------------------------
class _Block(nn.Module):
    """ResNet-style naming: conv<i> with bn<i> beside it, a Sequential(conv, bn) downsample, a biased plain convolution"""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(16, 32, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(32)
        self.conv2 = nn.Conv2d(32, 32, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(32)
        self.downsample = nn.Sequential(nn.Conv2d(16, 32, 1, stride=2, bias=False), nn.BatchNorm2d(32))
        self.out = nn.Conv2d(32, 13, 1)                      # 13 outputs: 1x1 with an even product
        self.odd = nn.Conv2d(32, 16, 5, padding=2)           # 5x5: never on the split kernels
        self.eval()


class _FakeTable(object):
    """numerics._Table with the reference in place of the kernel"""
    made = 0

    def __init__(self, tensors, scales, limits):
        _FakeTable.made += 1
        self.args = (tensors, scales, limits)

    def run(self):
        tensors, scales, (hi1, hi2) = self.args
        rows = []
        for t, sc in zip(tensors, scales):
            r = dict(v=t.detach().numpy(), hi1=hi1, hi2=hi2)
            if sc is not None:
                r.update(inner=sc.inner, var=sc.var.numpy(), eps=sc.eps, gamma=None if sc.gamma is None else sc.gamma.numpy())
            rows.append(r)
        return ref.records(rows)


@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(numerics, '_Table', _FakeTable)

    def no_library():
        raise AssertionError('the library was touched')
    monkeypatch.setattr(conv1x1, '_library', no_library)
    monkeypatch.delenv('KGDET_ENVELOPE', raising=False)
    yield
    conv1x1._bf16_parts.clear()


def test_enumeration_finds_pairs_plain_convolutions_and_rebuilds_on_pointer_change(fake):
    m = _Block()
    g = numerics.EnvelopeGuard(m)
    names = [l.name for l in g.layers]
    assert names == ['conv1 (folded)', 'conv2 (folded)', 'downsample.0 (folded)', 'conv1', 'conv2', 'downsample.0', 'out']
    assert [l.bn is not None for l in g.layers] == [True] * 3 + [False] * 4
    before = _FakeTable.made
    assert g.check() == [] and g.check() == []
    assert _FakeTable.made == before + 1                     # one table for both checks
    m.bn1.running_var = torch.ones(32)                       # another buffer object, another address
    assert g.check() == []
    assert _FakeTable.made == before + 2
    assert g.launches == 3


def _spoil(m):
    with torch.no_grad():
        m.conv2.weight.normal_(0, 1)
        m.bn2.running_var[7] = 1e-12                         # s = 316: |w s| far beyond 255.875 in channel 7 only
    return m


def test_check_names_the_layer_and_the_limit(fake):
    m = _spoil(_Block())
    v = numerics.EnvelopeGuard(m).check()
    assert [x.name for x in v] == ['conv2 (folded)'] and v[0].weight is m.conv2.weight
    w = m.conv2.weight.detach().numpy()
    expect = ref.record(w, numerics.WEIGHT_LIMIT, numerics.WEIGHT_CLAMP, inner=32 * 9, var=m.bn2.running_var.numpy(), eps=m.bn2.eps,
                        gamma=m.bn2.weight.detach().numpy())
    assert (np.float32(v[0].max), v[0].nonfinite, v[0].over1, v[0].over2) == expect
    assert v[0].limit == ('clamp' if expect[3] else 'limit') and v[0].over1 > 0
    assert 'conv2 (folded)' in numerics.describe(v[0])


def test_policy_bf16_routes_and_warns_once(fake):
    m = _spoil(_Block())
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        violations, rerouted = numerics.enforce(m)
        again = numerics.enforce(m)
    assert [v.name for v in rerouted] == ['conv2 (folded)'] and len(violations) == 1
    assert conv1x1.bf16_parts(m.conv2.weight) and not conv1x1.bf16_parts(m.conv1.weight)
    assert conv1x1.forward_f16(m.conv2.weight) is False and conv1x1.forward_f16(m.conv1.weight) == conv1x1.FORWARD_F16
    assert again[1] == [] and len(again[0]) == 1            # still outside, already routed: nothing to do, nothing said twice
    assert len([c for c in caught if 'conv2 (folded)' in str(c.message)]) == 1


def test_policy_raise_warn_and_nonfinite(fake, monkeypatch):
    m = _spoil(_Block())
    monkeypatch.setenv('KGDET_ENVELOPE', 'raise')
    with pytest.raises(numerics.EnvelopeError, match=r'conv2 \(folded\): max \|w s\| = '):
        numerics.enforce(m)
    assert not conv1x1.bf16_parts(m.conv2.weight)
    monkeypatch.setenv('KGDET_ENVELOPE', 'warn')
    with pytest.warns(RuntimeWarning, match='clamped'):
        assert numerics.enforce(m)[1] == []
    assert not conv1x1.bf16_parts(m.conv2.weight)
    with torch.no_grad():
        m.out.weight[3, 5] = float('nan')
    for mode in ('bf16', 'warn', 'raise'):
        monkeypatch.setenv('KGDET_ENVELOPE', mode)
        with pytest.raises(numerics.EnvelopeError, match='out: 1 non-finite'):
            numerics.enforce(m)
    monkeypatch.setenv('KGDET_ENVELOPE', 'bogus')
    with pytest.raises(ValueError):
        numerics.policy()


def test_policy_off_never_touches_the_library(fake, monkeypatch, tmp_path):
    made = _FakeTable.made
    m = _spoil(_Block())
    monkeypatch.setenv('KGDET_ENVELOPE', 'off')
    assert numerics.enforce(m) == ([], [])
    assert _FakeTable.made == made and not conv1x1.bf16_parts(m.conv2.weight)
    # a CPU model through load_checkpoint, under every policy: skipped before anything is scanned
    from kgdet_amd import checkpoint
    checkpoint.save_checkpoint(m, str(tmp_path / 'm.pth'))
    for mode in ('off', 'bf16', 'raise'):
        monkeypatch.setenv('KGDET_ENVELOPE', mode)
        checkpoint.load_checkpoint(_Block(), str(tmp_path / 'm.pth'))
    assert _FakeTable.made == made


def test_set_bf16_parts_remarks_images_and_drops_the_derived_state(fake, monkeypatch):
    import weakref
    from kgdet_amd import backbone
    m = _Block()
    w = m.conv2.weight
    e = conv1x1._FoldEntry()
    e.ref, e.bn, e.ptr, e.token = weakref.ref(w), weakref.ref(m.bn2), w.data_ptr(), 5
    e.img, e.img_t = conv1x1._mark(torch.empty(4, dtype=torch.uint8), True), conv1x1._mark(torch.empty(4, dtype=torch.uint8), False)
    e.s = e.t = None
    monkeypatch.setitem(conv1x1._fold_entries, id(w), e)
    monkeypatch.setattr(conv1x1, '_table', ('key', None, 0))
    monkeypatch.setattr(conv1x1, 'FORWARD_F16', True)
    hit = backbone._Folded(weakref.ref(m.conv2), None, None, None, None, None)
    other = backbone._Folded(weakref.ref(m.conv1), None, None, None, None, None)
    monkeypatch.setitem(backbone._fold_cache, (id(m.conv2), False), hit)
    monkeypatch.setitem(backbone._fold_cache, (id(m.conv1), False), other)
    assert conv1x1.set_bf16_parts(w) is True
    assert e.img.kgdet_f16 is False and e.img_t.kgdet_f16 is False and e.token == 0
    assert conv1x1._table is None
    assert (id(m.conv2), False) not in backbone._fold_cache and (id(m.conv1), False) in backbone._fold_cache
    assert conv1x1.set_bf16_parts(w) is False              # no change, nothing done
    assert conv1x1.set_bf16_parts(w, False) is True and e.img.kgdet_f16 is True
    # explicit formats win, defaults are today's
    assert conv1x1.forward_f16(w, True) is True and conv1x1.forward_f16(w, False) is False and conv1x1.forward_f16(w) is True


def test_a_captured_step_blocks_the_reroute(fake):
    class Step(object):
        pass
    m = _Block()
    step = Step()
    step.model = m
    conv1x1.register_capture(step)
    try:
        with pytest.raises(numerics.EnvelopeError, match='build the graphed step again'):
            conv1x1.set_bf16_parts(m.conv1.weight)
        assert conv1x1.set_bf16_parts(_Block().conv1.weight) is True      # another model's weight is free to move
        conv1x1.release_capture(step)
        assert conv1x1.set_bf16_parts(m.conv1.weight) is True
    finally:
        conv1x1.release_capture(step)
