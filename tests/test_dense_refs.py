"""tests/dense_refs.py pinned on the CPU: the restated operand split against independent casts, S3 against the exact integer
result, the split's own error against the figures the project documents, the lattice condition of every case the GPU tests run,
and the case table itself."""
import numpy as np
import pytest
import torch

from tests import dense_refs as R

f32 = np.float32
FMTS = [R.BF16, R.FP16]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.int32)


def _probe():
    rng = np.random.default_rng(7)
    v = np.concatenate([rng.standard_normal(4096) * 10.0 ** rng.uniform(-12, 5, 4096),
                        [0.0, -0.0, 257.0, 2049.0, 65504.0, 65519.9, 65520.0, 1e5, -2e5, 131008.0, 2.0 ** -14, 2.0 ** -24, 3e-8, 1e-30]])
    return v.astype(f32)


def test_bf16_split_is_round_to_nearest_even_twice():
    v = _probe()
    hi, lo = R.split(v, R.BF16)
    want_hi = R.bf16_round_bits(v)
    assert (_bits(hi.numpy()) == _bits(want_hi)).all()
    assert (_bits(lo.numpy()) == _bits(R.bf16_round_bits(v - want_hi))).all()
    # halfway cases go to the even neighbour: 257 = 256 + 1, 259 -> 260 - 1
    for x, h, l in ((257.0, 256.0, 1.0), (259.0, 260.0, -1.0), (-257.0, -256.0, -1.0)):
        hi, lo = R.split(f32(x), R.BF16)
        assert (float(hi), float(lo)) == (h, l)


def test_fp16_split_rounds_to_nearest_even_and_saturates():
    v = _probe()
    hi, lo = R.split(v, R.FP16)
    with np.errstate(over='ignore'):
        want_hi = np.clip(v.astype(np.float16).astype(f32), -R.F16_MAX, R.F16_MAX)
        want_lo = np.clip((v - want_hi).astype(np.float16).astype(f32), -R.F16_MAX, R.F16_MAX)
    assert (_bits(hi.numpy()) == _bits(want_hi)).all() and (_bits(lo.numpy()) == _bits(want_lo)).all()
    for x, h, l in ((2049.0, 2048.0, 1.0), (2051.0, 2052.0, -1.0), (1e5, 65504.0, 34496.0), (131008.0, 65504.0, 65504.0), (3e5, 65504.0, 65504.0),
                    (3e-8, 2.0 ** -24, 0.0)):                 # below half a subnormal quantum the lo part is gone
        hi, lo = R.split(f32(x), R.FP16)
        assert (float(hi), float(lo)) == (h, l), x
    wh, wl, scale = R.split_weight(f32(0.03), R.FP16)                    # dense_common.h: the lo part of 0.03 x 2^8 is normal
    assert scale == 2.0 ** -8 and abs(float(wl)) >= 2.0 ** -14 and float(wh) + float(wl) == pytest.approx(0.03 * 256, rel=2.0 ** -21)


def _lattice_operands():
    """(tag, op, a, b, fmt, q, extra of the epilogue) of every exact-tier case the GPU file runs"""
    for c in R.FWD_CASES:
        for fmt in ([R.BF16] if c.transpose else FMTS):
            la = R.fwd_lattice(c.name, fmt)
            extra = np.abs(la.bias.astype(np.float64)).reshape(1, -1, 1, 1) + np.abs(la.residual.astype(np.float64))
            yield 'fwd %s fmt%d' % (c.name, fmt), R.fwd_op(c), la.a, la.b, fmt, la.q, extra
    for s in R.S2GI_CASES:
        la = R.s2gi_lattice(*s)
        yield 's2gi %s' % (s,), R.op_grad_input(3, 2, s[3], s[4]), la.a, la.b, R.BF16, la.q, 0.0
    for s in R.STEM_CASES:
        for fmt in FMTS:
            la = R.stem_lattice(*s, fmt)
            yield 'stem %s fmt%d' % (s, fmt), R.op_forward(7, 2), la.a, la.b, fmt, la.q, 0.0
    for c in R.GW_CASES:
        gl = R.gw_lattice(c.name)
        yield 'gw %s' % c.name, R.gw_op(c), gl.gy, gl.x, R.BF16, gl.q, 0.0


def test_lattice_condition_holds_for_every_gpu_case():
    """every term a multiple of q (operands are integers times powers of two with exact splits) and sum |terms| < 2^24 q"""
    n = 0
    for tag, op, a, b, fmt, q, extra in _lattice_operands():
        for t in (a, b):
            scaled = R.split_weight(t, fmt) if (t is b and op.b_is_weight) else R.split(t, fmt) + (1.0,)
            assert torch.equal((scaled[0] + scaled[1]).double() * scaled[2], torch.as_tensor(t).double()), tag      # hi + lo == v
            assert bool((scaled[1] != 0).any()), tag + ': no wide value'
        assert R.lattice_ok(R.abs_terms(op, a, b, fmt).numpy(), q, extra), tag
        n += 1
    assert n == 2 * len(R.FWD_CASES) - sum(c.transpose for c in R.FWD_CASES) + len(R.S2GI_CASES) + 2 * len(R.STEM_CASES) + len(R.GW_CASES)
    for c in R.GW_CASES:             # grad_beta: the per-row sums of grad_y, and bn_partial's
        gl = R.gw_lattice(c.name)
        assert np.abs(gl.gy.astype(np.float64)).sum(axis=(0, 2, 3)).max() < 2.0 ** 24 * 2.0 ** R.EG
        assert np.abs(gl.bn_partial.astype(np.float64)).sum(1).max() < 2.0 ** 24 * 2.0 ** R.EG


SMALL = ['fwd nn1_store fmt0', 'fwd nn1_store fmt1', 'fwd nn9_s2_ks2 fmt1', 'fwd p44_store fmt0', 'fwd p44_store fmt1', 'fwd gi9 fmt0',
         's2gi (1, 72, 32, 13, 11)', 'stem (2, 37, 45) fmt0', 'stem (2, 37, 45) fmt1', 'gw ntp9_ragged', 'gw nt8_1', 'gw s2_ragged']


def test_s3_is_the_exact_integer_result_minus_the_dropped_product():
    seen = set()
    for tag, op, a, b, fmt, q, _ in _lattice_operands():
        if tag not in SMALL:
            continue
        seen.add(tag)
        s3, ex, ll = (f(op, a, b, *r).numpy() for f, r in ((R.s3, (fmt,)), (R.exact, ()), (R.lolo, (fmt,))))
        assert (np.round(ex / q) * q == ex).all() and np.abs(ll).max() > 0, tag           # integers; wide values met wide values
        assert (_bits(s3) == _bits(ex - ll)).all(), tag
        assert (s3.astype(f32).astype(np.float64) == s3).all(), tag                        # ... and S3 is a float32 number
        assert (s3 != ex).any(), tag
    assert seen == set(SMALL)


@pytest.mark.parametrize('fmt', FMTS)
def test_split_error_at_unit_scale_stays_inside_the_documented_figures(fmt):
    """dense_common.h: ~5e-6 of the output scale for bf16 parts; include/kgdet_hip.h: <= 1e-6 for fp16 parts.  The operands of the
    existing dense tests: randn activations, 0.1 randn weights."""
    g = torch.Generator().manual_seed(0)
    worst = 0.0
    for k, K in ((1, 256), (3, 64), (3, 512)):
        x, w = torch.randn(1, K, 12, 14, generator=g), 0.1 * torch.randn(128, K, k, k, generator=g)
        op = R.op_forward(k, 1)
        ex = R.exact(op, x, w)
        worst = max(worst, float((R.s3(op, x, w, fmt) - ex).abs().max() / ex.abs().max()))
    print('S3 - exact at unit scale, fmt %d: %.3g of the output scale' % (fmt, worst))
    assert worst <= {R.BF16: 5e-6, R.FP16: 1e-6}[fmt]


def _backward_mixed():
    """(name, op, a, b, group axis) of every mixed-scale backward case"""
    for c in R.GW_CASES:
        yield (c.name, R.gw_op(c)) + R.gw_mixed(c.name) + (0,)
    for c in R.FWD_CASES:
        if c.transpose:
            yield (c.name, R.fwd_op(c)) + R.fwd_mixed(c.name) + (0,)
    for s in R.S2GI_CASES:
        yield ('s2gi %s' % (s,), R.op_grad_input(3, 2, s[3], s[4])) + R.s2gi_mixed(*s) + (0,)


def test_bf16_backward_split_at_gradient_magnitude():
    """the envelope tier's premise: at 1e-8 and below every bf16 part is still a normal number, so S3 is what it is at unit scale
    (the same grad_y times 2^40: bit for bit after rescaling), and per group it leaves the accumulation bar of room under 1e-5 --
    except in the cases named in dense_refs.BF16_SPLIT_OVER, whose figures are pinned here"""
    seen = set()
    for name, op, a, b, axis in _backward_mixed():
        s3 = R.s3(op, a, b, R.BF16)
        big = (torch.as_tensor(a).double() * 2.0 ** 40).float()
        assert torch.equal(s3 * 2.0 ** 40, R.s3(op, big, b, R.BF16)), name
        r = R.group_ratio(s3.numpy(), R.exact(op, a, b).numpy(), axis)
        print('S3 - exact per group, %s: %.3g' % (name, r))
        if name in R.BF16_SPLIT_OVER:
            seen.add(name)
            assert R.ENVELOPE_ROOM < r <= R.BF16_SPLIT_OVER[name], (name, r)
        else:
            assert r <= R.ENVELOPE_ROOM, (name, r)
    assert seen == set(R.BF16_SPLIT_OVER)


def test_fp16_weight_rows_below_the_normal_lo_range_lose_bits():
    """What the fp16 image keeps of a weight row far below the others (a BatchNorm fold scale near zero).  Above |w| ~ 2^-11 the lo
    part of w x 2^8 is a normal fp16 number and a row keeps the documented 1e-6 of ITS OWN output scale; below, the lo part is
    subnormal (quantum 2^-24) and the row's error grows as its weights shrink.  Measured here, documented in include/kgdet_hip.h."""
    c = R.FWD_BY_NAME['nn1_ks2_uneven']
    x, w = R.fwd_mixed(c.name)
    op = R.fwd_op(c)
    ex, s3 = R.exact(op, x, w).numpy(), R.s3(op, x, w, R.FP16).numpy()
    err = np.abs(s3 - ex).max(axis=(0, 2, 3)) / np.abs(ex).max(axis=(0, 2, 3))
    rms = np.sqrt((w.astype(np.float64) ** 2).mean(axis=(1, 2, 3)))
    inside = rms >= 4 * R.F16_WEIGHT_NORMAL_LO            # (nearly) every weight of the row above 2^-11
    assert inside.sum() >= 20 and (~inside).sum() >= 20
    print('fp16 parts, S3 - exact per row: %.3g inside, %.3g below (row rms down to %.3g)' % (err[inside].max(), err[~inside].max(), rms.min()))
    assert err[inside].max() <= R.SPLIT_BAR[R.FP16]
    # below: the absolute floor of the image, half a subnormal quantum per weight, 2^-25 / 2^8, against the row's own scale
    K = w[0].size
    floor = 2.0 ** -33 * np.sqrt(K) * 4.0 / (rms * np.sqrt(K))         # ~4 sigma of K independent roundings over the row's output sigma
    assert (err[~inside] <= np.maximum(floor[~inside], R.SPLIT_BAR[R.FP16])).all()
    assert err[~inside].max() > R.SPLIT_BAR[R.FP16]                      # the finding: such rows are NOT fp32-class


def test_generators_are_deterministic():
    for make, args in ((R.fwd_lattice, ('p44_ks2', R.FP16)), (R.gw_lattice, ('ntp9_ragged',)), (R.fwd_mixed, ('gi9',)),
                       (R.gw_mixed, ('nt8_1',)), (R.s2gi_lattice, R.S2GI_CASES[0]), (R.stem_lattice, R.STEM_CASES[0] + (R.BF16,))):
        a = make(*args)
        make.cache_clear()
        b = make(*args)
        assert a is not b
        for u, v in zip(a, b):
            assert (u is None and v is None) or np.array_equal(np.asarray(u), np.asarray(v))


def test_case_table():
    plans = [(c.kernel, c.ks, c.closer, c.stride, c.transpose, c.kernel == 'p24' and c.M <= 64) for c in R.FWD_BRANCHES]     # (p24: both reasons)
    assert len(set(plans)) == len(plans)
    assert {c.kernel for c in R.FWD_BRANCHES} == {'nn1w4', 'nn1w5', 'nn9w4', 'nn9w5', 'p44', 'p24', 'p45'}
    assert {c.closer for c in R.FWD_BRANCHES} == {0, 1, 2}
    for e in R.FWD_EDGES:
        assert any((e.kernel, e.stride) == (c.kernel, c.stride) for c in R.FWD_BRANCHES), e.name
    rows = [(c.route, c.product, c.splits > 1) for c in R.GW_CASES]
    assert len(set(rows)) == len(rows)
    assert {(c.route, c.product) for c in R.GW_CASES} >= {('1x1', 'nt8'), ('1x1', 'ntp_ragged'), ('1x1', 'nt8_padded'), ('3x3', 'ntp_aligned'),
                                                          ('3x3', 'ntp_ragged'), ('3x3', 'nt8_padded'), ('s2', 'nt8'), ('s2', 'ntp_ragged')}
    closers = {(c.route, k) for c in R.GW_CASES for k in c.closers}
    assert closers == {(r, k) for r, ks in (('1x1', ('sum', 'fold', 'fold_rows')), ('3x3', ('wsum', 'fold', 'fold_rows')), ('s2', ('wsum',))) for k in ks}
    names = [c.name for c in R.FWD_CASES] + [c.name for c in R.GW_CASES]
    assert len(set(names)) == len(names)
    assert set(R.CLOSER_CASES) <= set(R.FWD_BY_NAME)
    for c in R.FWD_CASES:            # what the ABI asks of a shape
        assert c.taps == 1 or c.K % 16 == 0
        assert c.ks == 1 or (c.B * c.M * -(-c.H // c.stride) * -(-c.W // c.stride)) % 2 == 0
    for c in R.GW_CASES:
        assert c.route == '1x1' and c.H == 1 or c.route != '1x1'
        assert c.route != '3x3' or c.C % 128 == 0
        assert (c.O * c.C) % 2 == 0
