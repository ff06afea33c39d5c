"""tests/grouped_conv_nhwc_refs.py held to independent statements, and the host side of the bf16 channels-last grouped
convolution (kgdet_amd/grouped_conv.py applicable_bf16 / BF16, the refusals of kgdet_gconv3x3_nhwc_bf16) -- no GPU."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import grouped_conv_nhwc_refs as R

E_SHAPE = 1


# ---------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize('cpg,stride,groups,B,H,W', [(4, 1, 6, 2, 5, 7), (8, 2, 3, 1, 7, 6), (16, 2, 1, 3, 1, 7), (32, 1, 3, 1, 8, 8)])
def test_float64_sum_is_conv2d_on_permuted_operands(cpg, stride, groups, B, H, W):
    rng = np.random.default_rng([cpg, stride, 5])
    C = groups * cpg
    x = torch.from_numpy(rng.standard_normal((B, C, H, W))).contiguous(memory_format=torch.channels_last)
    w = torch.from_numpy(rng.standard_normal((C, cpg, 3, 3))).contiguous(memory_format=torch.channels_last)
    want = F.conv2d(x, w, None, stride, 1, 1, groups).permute(0, 2, 3, 1).numpy()
    # (the storage of a channels-last tensor IS the packed layout: the permuted views below copy nothing)
    x_nhwc, w_packed = x.permute(0, 2, 3, 1).numpy(), w.permute(0, 2, 3, 1).numpy()
    assert x_nhwc.flags['C_CONTIGUOUS'] and w_packed.flags['C_CONTIGUOUS']
    assert np.array_equal(R.pack_weight(w.numpy()), w_packed) and np.array_equal(R.to_nhwc(x.numpy()), x_nhwc)
    got = R.sum64(x_nhwc, w_packed, stride)
    assert got.shape == want.shape == (B, R.out_size(H, stride), R.out_size(W, stride), C)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_case_table_covers_the_issue_and_the_kernels_seams():
    seen = {(c.cpg, c.stride, c.H, c.W) for c in R.CASES}
    for cpg in R.CPGS:
        for stride in (1, 2):
            for m in R.SMALL_MAPS + R.LARGE_MAPS:
                assert (cpg, stride) + m in seen
        assert {c.groups for c in R.CASES if c.cpg == cpg and c.name.startswith('c')} >= set(R.GROUPS[cpg])
    assert {c.B for c in R.CASES} >= {1, 3}
    assert all((c.groups * c.cpg) % 8 == 0 for c in R.CASES)
    assert any((c.groups * c.cpg) % 16 == 8 for c in R.CASES) and any(c.groups * c.cpg > 64 for c in R.CASES)
    # the second trip of a workgroup: more tiles than the 4096 workgroups of a one-slab launch
    for c in R.CASES:
        if c.name.startswith('trip_'):
            th = 8 if c.stride == 1 else 4
            tiles = c.B * -(-R.out_size(c.H, c.stride) // th) * -(-R.out_size(c.W, c.stride) // 16)
            assert c.groups * c.cpg <= 64 and tiles > 4096


@pytest.mark.parametrize('name', R.NAMES)
def test_lattice_cases_have_every_partial_sum_exact(name):
    c, op = R.BY_NAME[name], R.lattice(name)
    q = 2.0 ** (R.XE + R.WE)
    for v, e in ((op.x, R.XE), (op.w, R.WE), (op.bias, R.BE)):
        n = v.astype(np.float64) / 2.0 ** e
        assert (n == np.round(n)).all() and np.abs(n).max() <= 3
        R.bf16_bits(v)                                   # bf16 numbers
    S, worst = R.lattice_sum(name)
    assert worst <= 9 * c.cpg * 9 <= 9 * 32 * 9 < 2 ** 24
    assert (S / q == np.round(S / q)).all() and (S.astype(np.float32).astype(np.float64) == S).all()
    # the epilogue's addition is exact in float32 too: bf16(S) and the bias are multiples of 2^-9 below 2^4
    t = R.final_raw(S).astype(np.float64) + op.bias.astype(np.float64)
    assert (t.astype(np.float32).astype(np.float64) == t).all()


def test_a_lattice_case_rounds_a_tie():
    counts = {name: R.ties(name) for name in R.NAMES if not name.startswith('trip_')}
    print('ties per case:', {k: v for k, v in counts.items() if v})
    assert sum(1 for v in counts.values() if v) >= 1
    # round to nearest EVEN there: the reference's rounding differs from rounding half up or half away on some tie
    name = max(counts, key=counts.get)
    S, _ = R.lattice_sum(name)
    s32 = S.astype(np.float32)
    u = s32.view(np.uint32)
    tie = (u & 0xffff) == 0x8000
    got = R.bf16_bits(R.final_raw(S))[tie]
    assert ((got & 1) == 0).all() and (got != ((u[tie] + 0x8000) >> 16)).any()


def test_final_maps():
    s = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.75, 2.0 ** -20])
    assert np.array_equal(R.final_raw(s), np.array([1.0, 1.0 + 2.0 ** -6, -0.75, 2.0 ** -20], np.float32))
    bias = np.array([0.5, -2.0, 0.5, 0.0], np.float32)
    assert np.array_equal(R.final_epilogue(s, bias), np.array([1.5, -1.0 + 2.0 ** -6, -0.25, 2.0 ** -20], np.float32))
    assert np.array_equal(R.final_epilogue(s, bias, relu=True), np.array([1.5, 0.0, 0.0, 2.0 ** -20], np.float32))
    assert np.array_equal(R.final_epilogue(s, None, relu=True), np.array([1.0, 1.0 + 2.0 ** -6, 0.0, 2.0 ** -20], np.float32))
    assert np.array_equal(R.from_bf16_bits(R.bf16_bits(R.final_raw(s))), R.final_raw(s))


@pytest.mark.parametrize('cpg,stride', R.MIXED_CASES)
def test_mixed_ambiguous_shares_match_the_pinned_table(cpg, stride):
    iv = R.mixed_interval(cpg, stride)
    for mode, pinned in zip(R.MIXED_MODES, R.MIXED_AMBIGUOUS[(cpg, stride)]):
        share = iv[mode]['ambiguous']
        print('cpg %d stride %d %s: ambiguous share %.4f (pinned %.3f)' % (cpg, stride, mode, share, pinned))
        assert abs(share - pinned) <= 0.002 and share < R.MIXED_CAP


# ---------------------------------------------------------------------------------------------- applicable_bf16, the switch
def test_applicable_bf16_refuses_what_the_kernel_does_not_take(monkeypatch):
    from kgdet_amd import grouped_conv
    monkeypatch.setattr(grouped_conv, 'BF16', 'force')
    monkeypatch.setattr(grouped_conv, 'ENABLED', True)
    cl = torch.channels_last
    with torch.no_grad():
        x = torch.zeros(1, 16, 5, 7, dtype=torch.bfloat16).contiguous(memory_format=cl)
        w = torch.zeros(16, 4, 3, 3, dtype=torch.bfloat16).contiguous(memory_format=cl)
        args = ((1, 1), (1, 1), (1, 1), 4)
        assert grouped_conv.shape_ok(x.shape, w.shape, *args)
        assert not grouped_conv.applicable_bf16(x, w, *args)                           # CPU tensors
        assert not grouped_conv.applicable_bf16(x.float(), w.float(), *args)           # fp32
        # every other condition on stand-ins that claim to be on the GPU, so that the device test does not answer for them
        fx, fw = _Fake(x), _Fake(w)
        assert grouped_conv.applicable_bf16(fx, fw, *args)
        assert not grouped_conv.applicable_bf16(_Fake(x.float()), _Fake(w.float()), *args)       # fp32
        assert not grouped_conv.applicable_bf16(_Fake(x.contiguous()), fw, *args)                # NCHW activation
        assert not grouped_conv.applicable_bf16(fx, _Fake(w.contiguous()), *args)                # NCHW weight
        x12 = torch.zeros(1, 12, 5, 7, dtype=torch.bfloat16).contiguous(memory_format=cl)
        w12 = torch.zeros(12, 4, 3, 3, dtype=torch.bfloat16).contiguous(memory_format=cl)
        assert grouped_conv.shape_ok(x12.shape, w12.shape, (1, 1), (1, 1), (1, 1), 3)
        assert not grouped_conv.applicable_bf16(_Fake(x12), _Fake(w12), (1, 1), (1, 1), (1, 1), 3)   # C % 8 != 0
        assert not grouped_conv.applicable_bf16(fx, fw, (1, 1), (1, 1), (2, 2), 4)               # dilation
        assert not grouped_conv.applicable_bf16(fx, fw, (3, 3), (1, 1), (1, 1), 4)               # stride
    with torch.enable_grad():
        assert not grouped_conv.applicable_bf16(fx, fw, *args)                                   # grad mode


class _OnGpu(torch.Tensor):
    """a CPU tensor that answers ``is_cuda`` with True (applicable_bf16 reads attributes and launches nothing)"""
    is_cuda = property(lambda self: True)


def _Fake(t):
    return t.as_subclass(_OnGpu)


def test_switch_parsing_and_classes(monkeypatch):
    from kgdet_amd import grouped_conv
    assert grouped_conv.parse_bf16(None) == grouped_conv.parse_bf16('') == grouped_conv.parse_bf16('0') == '0'
    assert grouped_conv.parse_bf16('1') == '1' and grouped_conv.parse_bf16('force') == 'force'
    for bad in ('2', 'on', 'FORCE'):
        with pytest.raises(ValueError):
            grouped_conv.parse_bf16(bad)
    assert set(grouped_conv.calls) == {'forward', 'bias_act', 'grad_input', 'grad_weight'}
    assert set(grouped_conv.calls_nhwc) == {'raw', 'bias_act'}
    grouped_conv.calls_nhwc['raw'] += 2
    grouped_conv.reset_calls_nhwc()
    assert grouped_conv.calls_nhwc == {'raw': 0, 'bias_act': 0}
    cl = torch.channels_last
    x = _Fake(torch.zeros(1, 32, 5, 7, dtype=torch.bfloat16).contiguous(memory_format=cl))
    w = _Fake(torch.zeros(32, 16, 3, 3, dtype=torch.bfloat16).contiguous(memory_format=cl))
    args = ((2, 2), (1, 1), (1, 1), 2)
    with torch.no_grad():
        monkeypatch.setattr(grouped_conv, 'ENABLED', True)
        monkeypatch.setattr(grouped_conv, 'TORCH_CLASSES_BF16', frozenset([(16, 2)]))
        for setting, want in (('0', False), ('1', False), ('force', True)):
            monkeypatch.setattr(grouped_conv, 'BF16', setting)
            assert grouped_conv.applicable_bf16(x, w, *args) is want
        monkeypatch.setattr(grouped_conv, 'TORCH_CLASSES_BF16', frozenset([(16, 1)]))
        monkeypatch.setattr(grouped_conv, 'BF16', '1')
        assert grouped_conv.applicable_bf16(x, w, *args)
        monkeypatch.setattr(grouped_conv, 'ENABLED', False)          # KGDET_GROUPED_CONV=0 turns this route off as well
        monkeypatch.setattr(grouped_conv, 'BF16', 'force')
        assert not grouped_conv.applicable_bf16(x, w, *args)


def test_the_default_is_off():
    import os
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k != 'KGDET_GROUPED_CONV_BF16'}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = 'from kgdet_amd import grouped_conv as g; print(g.BF16, len(g.TORCH_CLASSES_BF16) >= 0)'
    assert subprocess.check_output([sys.executable, '-c', code], cwd=root, env=env).decode().split()[0] == '0'
    env['KGDET_GROUPED_CONV_BF16'] = 'force'
    assert subprocess.check_output([sys.executable, '-c', code], cwd=root, env=env).decode().split()[0] == 'force'


# ---------------------------------------------------------------------------------------------- the C ABI's refusals
def _entry():
    from kgdet_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, 'kgdet_gconv3x3_nhwc_bf16'), 'libkgdet_hip.so has no kgdet_gconv3x3_nhwc_bf16'
    fn = L.kgdet_gconv3x3_nhwc_bf16
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    fn.restype, fn.argtypes = ctypes.c_int, [vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, vp]
    L.kgdet_last_error.restype = ctypes.c_char_p
    return L, fn


# addresses that are never dereferenced: every call below is refused by host code before any launch
X, W_, BIAS, Y = 0x10000000, 0x20000000, 0x30000000, 0x40000000
GOOD = dict(x=X, w=W_, bias=BIAS, y=Y, B=2, C=32, cpg=8, H=5, W=7, stride=1, relu=1)
REFUSALS = [
    ('another cpg', dict(cpg=2, C=32)), ('cpg 64', dict(cpg=64, C=64)), ('cpg 12', dict(cpg=12, C=24)),
    ('stride 3', dict(stride=3)), ('stride 0', dict(stride=0)),
    ('C % cpg', dict(C=40, cpg=16)), ('C % 8', dict(C=12, cpg=4)), ('C % 8, one group', dict(C=4, cpg=4)),
    ('null x', dict(x=None)), ('null w', dict(w=None)), ('null y', dict(y=None)),
    ('misaligned x', dict(x=X + 8)), ('misaligned w', dict(w=W_ + 2)), ('misaligned bias', dict(bias=BIAS + 4)),
    ('misaligned y', dict(y=Y + 8)),
    ('y is x', dict(y=X)), ('y inside x', dict(y=X + 16)), ('y reaches w', dict(y=W_ - 16)), ('y on the bias', dict(y=BIAS + 64)),
    ('empty batch', dict(B=0)), ('empty map', dict(H=0)),
]


@pytest.mark.parametrize('what,change', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_point_exists_and_refuses_from_the_host(what, change):
    L, fn = _entry()
    a = dict(GOOD, **change)
    rc = fn(a['x'], a['w'], a['bias'], a['y'], a['B'], a['C'], a['cpg'], a['H'], a['W'], a['stride'], a['relu'], None)
    assert rc == E_SHAPE, what
    assert b'gconv3x3_nhwc_bf16' in L.kgdet_last_error(), what
