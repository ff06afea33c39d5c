"""tests/nhwc_refs.py held to its own claims on the CPU, before a GPU is involved: the lattice condition that makes the exact tier
order-independent, each of the three roundings visibly at work, six deliberately wrong kernels each told apart from the right one,
and the mixed-scale tier's ambiguous share as pinned -- so a mismatch in tests/test_gpu_nhwc_kernels.py is a finding about the kernel.

The three persistent-loop shapes (M of 16389 .. 196609 rows) are evaluated in full for the roundings' rates and the headroom bound;
the defects, over all the combinations they apply to, on their first and last 512 rows: every row is an independent draw of the same
distribution and a defect acts row by row.
"""
import numpy as np
import pytest

from tests import nhwc_refs as R

ALL_ON = (1, 1, 1)


def _rows(case):
    """the rows the per-combination checks read: all of a small case, both ends of a large one"""
    return [slice(None)] if case in R.SMALL_CASES else [slice(0, 512), slice(case[2] - 512, case[2])]


def test_cases_are_what_the_table_says():
    assert len(R.EXACT_CASES) == 13 and len(set(R.EXACT_CASES)) == 13 and len(R.COMBOS) == 8
    for K, N, M in R.EXACT_CASES:
        assert K % 16 == 0 and K <= 512 and (N % 128 == 0 or N == 64)
    waves = lambda K: 8 if 256 <= K <= 384 else 4
    # second trip of workgroup 0 = the one ragged row tile behind 768 full ones
    for K, N, M in R.LARGE_CASES[:2]:
        rows = 32 * waves(K)
        assert (M + rows - 1) // rows == 769 and M % rows == 1
    K, N, M = R.LARGE_CASES[2]        # K > 384: 256 / n_ctiles workgroups per column tile
    assert K > 384 and N == 256 and (M + 127) // 128 > 256 // (N // 128) and M % 128 == 5
    for K, N in R.REFUSED:
        assert K % 16 or K > 512 or not (N % 128 == 0 or N == 64)


@pytest.mark.parametrize('case', R.EXACT_CASES, ids=R.case_id)
def test_lattice_condition(case):
    """sum_k |a w| + |bias| + |res| < 2^24 q on every element: by the bound over any draw for all rows, and measured"""
    K, N, M = case
    assert R.worst_case_magnitude(K) < 2 ** 24
    inp = R.exact_inputs(case)
    for name, unit in (('x0', R.X_UNIT), ('w', R.W_UNIT), ('in_bias', R.IB_UNIT), ('bias', R.Q), ('res', R.RES_UNIT)):
        v = inp[name].astype(np.float64) / unit
        assert (v == np.rint(v)).all(), name
    for name in ('x0', 'w', 'res'):                                      # what the kernel takes as bf16 is bf16
        R.bf16_bits(inp[name])
    R.bf16_bits(R.activation(inp, 0, slice(0, 512)))
    for combo in R.COMBOS:
        for rows in _rows(case):
            head = R.exact_headroom(case, combo, rows)
            assert head <= R.worst_case_magnitude(K)
            assert head < 0.03 * 2 ** 24, (combo, head / 2 ** 24)


@pytest.mark.parametrize('case', R.SMALL_CASES, ids=R.case_id)
def test_float32_evaluation_is_the_float64_one(case):
    """the reference's float32 sums are exact under the lattice condition: bit-equal to float64 at every stage"""
    for combo in R.COMBOS:
        a, b = R.exact_reference(case, combo), R.exact_reference(case, combo, dtype=np.float64)
        for k in ('a', 'S', 'Sr', 'f', 'out'):
            assert a[k].dtype == np.float32
            assert (a[k].astype(np.float64) == b[k]).all(), (combo, k)
        assert not np.signbit(a['out'][a['out'] == 0]).any()            # a zero is +0


@pytest.mark.parametrize('case', R.EXACT_CASES, ids=R.case_id)
def test_every_rounding_is_at_work(case):
    """each rounding changes at least 5 % of the elements it applies to (measured: input epilogue 12 .. 19 %, product 71 .. 95 %,
    final 46 .. 99 %)"""
    for combo in R.COMBOS if case in R.SMALL_CASES else [ALL_ON]:
        r = R.exact_reference(case, combo)
        rates = dict(product=float((r['S'] != r['Sr']).mean()), final=float((r['f'] != r['out']).mean()))
        if combo[1]:
            rates['input'] = float((r['pre_a'] != r['a']).mean())
        print('NHWC-ROUND %s %s %s' % (R.case_id(case), R.combo_id(combo), rates))
        assert min(rates.values()) >= 0.05, (combo, rates)
        assert np.isfinite(r['out']).all()


@pytest.mark.parametrize('defect', R.DEFECTS)
@pytest.mark.parametrize('case', R.EXACT_CASES, ids=R.case_id)
def test_defects_are_seen(case, defect):
    """each deliberately wrong kernel changes at least 1 % of the outputs of every (shape, combination) it applies to"""
    seen = 0
    for combo in R.COMBOS:
        if not R.defect_applies(defect, case, combo):
            continue
        for rows in _rows(case):
            good = R.exact_reference(case, combo, rows=rows)['out']
            bad = R.exact_reference(case, combo, defect=defect, rows=rows)['out']
            share = float((R.bf16_bits(good) != R.bf16_bits(bad)).mean())
            assert share >= 0.01, (combo, share)
            seen += 1
    K, N, M = case
    assert seen > 0 or (defect == 'halves_swapped' and N == 64)


def test_mixed_cases_cover_every_instantiation():
    assert len(R.MIXED_AMBIGUOUS) == len(R.MIXED_K) * len(R.COMBOS)
    for K in R.MIXED_K:
        got = {(relu, in_epi) for k, (relu, in_epi, _) in R.MIXED_CASES if k == K}
        want = {(1, 0), (1, 1)} if K == 512 else {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert got == want, K


@pytest.mark.parametrize('K', R.MIXED_K)
def test_mixed_ambiguous_share_is_as_pinned(K):
    for combo in R.COMBOS:
        iv = R.mixed_interval(K, combo)
        pinned = R.MIXED_AMBIGUOUS[(K, combo)]
        print('NHWC-AMBIGUOUS K%d %s %.4f (pinned %.4f)' % (K, R.combo_id(combo), iv['ambiguous'], pinned))
        assert abs(iv['ambiguous'] - pinned) <= 0.002
        if (K, combo) in R.MIXED_CASES:
            assert iv['ambiguous'] < R.MIXED_CAP
        assert np.isfinite(iv['lo']).all() and np.isfinite(iv['hi']).all() and (iv['lo'] <= iv['hi']).all()


def test_mixed_interval_holds_a_serial_float32_accumulation():
    """the plainest correct kernel -- float32, k ascending -- lies inside its interval, and outside it once a k-step is dropped"""
    K, combo = 128, (1, 1, 1)
    inp, iv = R.mixed_inputs(K), R.mixed_interval(K, combo)
    a = R.bf16_round_bits(np.maximum(inp['x'] + inp['in_bias'], np.float32(0)))
    acc = np.zeros((R.MIXED_M, R.MIXED_N), np.float32)
    for k in range(K):
        acc += a[:, k:k + 1] * inp['w'][:, k][None, :]
    out = R.mixed_final(acc.astype(np.float64), inp, combo)
    assert ((iv['lo'] <= out) & (out <= iv['hi'])).all()
    for k in range(K - 16, K):
        acc -= a[:, k:k + 1] * inp['w'][:, k][None, :]
    bad = R.mixed_final(acc.astype(np.float64), inp, combo)
    assert (~((iv['lo'] <= bad) & (bad <= iv['hi']))).mean() > 0.2
