"""tests/dcn_edge_cases.py held to its own claims on the CPU, before a GPU is involved: every shape of the table reaches every class
of sampling position, the float32 and the float64 evaluation of a position agree bit for bit, and the float32 oracle (the
reference's arithmetic) agrees with the float64 oracle on these inputs with NO element left out -- so a mismatch in
tests/test_gpu_dcn_edges.py is a finding about a kernel, never about a position that rounds differently in two precisions."""
import numpy as np
import pytest

from tests import dcn_edge_cases as E

SEED = 7
# float32 oracle against float64 oracle, as a fraction of each result's scale.  Measured with this construction: at most 6.2e-7
# (grad_input of the grouped 38 x 36 shape, v1; y of the 5x5 shape 5.8e-7; each test prints its numbers), so 2e-6 is about 3x over
# what the reference's own float32 arithmetic does and 10x under the tightest tolerance of the GPU tests.
ORACLE_TOL = 2e-6


@pytest.mark.parametrize('case', E.CASES, ids=E.case_id)
def test_every_class_of_position_is_hit_in_both_axes(case):
    off = E.edge_offsets(case, SEED)
    N, C, H, W, O, k, s, p, d, g, dg = case
    Ho, Wo = E.output_size(case)
    assert off.dtype == np.float32 and off.shape == (N, dg * 2 * k * k, Ho, Wo)
    assert np.isfinite(off).all()
    counts = E.classify(case, off)
    impossible = E.impossible_classes(case)
    # (the only classes a shape of the table rules out: fractions strictly inside (0, L-1) on an axis of length 1)
    assert impossible == {'y': {'inside_off_lattice'} if H == 1 else set(), 'x': set()}
    for axis in ('y', 'x'):
        for cls in E.CLASSES:
            if cls in impossible[axis]:
                assert counts[axis][cls] == 0, (axis, cls)
            else:
                assert counts[axis][cls] > 0, (axis, cls, counts[axis])


@pytest.mark.parametrize('case', E.CASES, ids=E.case_id)
def test_special_offsets_are_what_they_claim(case):
    N, C, H, W, O, k, s, p, d, g, dg = case
    sites = N * dg * k * k * int(np.prod(E.output_size(case)))
    out = E.classify(case, E.all_outside(case))
    assert out['y']['outside'] == sites and out['x']['outside'] == sites
    lat = E.classify(case, E.lattice(case))
    for axis in ('y', 'x'):     # undeformed positions: whole numbers, in the map or in its padding
        assert lat[axis]['lattice'] + lat[axis]['on_-1'] + lat[axis]['on_L'] + lat[axis]['outside'] == sites
        assert lat[axis]['lattice'] > 0
    m = E.edge_mask(case, SEED)
    assert m.dtype == np.float32 and m.min() == 0.0 and m.max() == 1.0
    assert 0.19 < float((m == 0).mean()) < 0.22 and (m == 1).sum() >= 3
    assert E.edge_offsets(case, SEED).tobytes() == E.edge_offsets(case, SEED).tobytes()   # fixed seeds: the same inputs every run


@pytest.mark.parametrize('case', E.CASES, ids=E.case_id)
def test_float32_positions_equal_float64_positions_bit_for_bit(case):
    N, C, H, W, O, k, s, p, d, g, dg = case
    off = E.edge_offsets(case, SEED)
    p32, p64 = E.positions(case, off, np.float32), E.positions(case, off, np.float64)
    for a32, a64, L in zip(p32, p64, (H, W)):
        assert a32.dtype == np.float32 and a64.dtype == np.float64
        near = (a64 >= -8) & (a64 <= L + 8)
        assert near.mean() > 0.5
        assert np.array_equal(a32[near].astype(np.float64), a64[near])
        # the rest is far outside in both precisions (same side, too)
        assert ((a32[~near] < -1) == (a64[~near] < -1)).all() and ((a32[~near] > L) == (a64[~near] > L)).all()
        assert ((a32[~near] < -1) | (a32[~near] > L)).all()


@pytest.mark.parametrize('v2', [False, True], ids=['v1', 'v2'])
@pytest.mark.parametrize('case', E.CASES, ids=E.case_id)
def test_float32_oracle_agrees_with_float64_oracle_everywhere(case, v2):
    r32 = E.reference(case, 'edge', v2, SEED, np.float32)
    r64 = E.reference(case, 'edge', v2, SEED, np.float64)
    names = ['y', 'grad_input', 'grad_offset', 'grad_weight'] + (['grad_mask', 'grad_bias'] if v2 else [])
    errs = {}
    for name in names:
        a, b = r32[name], r64[name]
        assert a.dtype == np.float32 and b.dtype == np.float64 and a.shape == b.shape
        scale = max(float(np.abs(b).max()), 1e-6)
        errs[name] = float(np.abs(a.astype(np.float64) - b).max()) / scale     # every element: no allowance
    print('%s %s: %s' % (E.case_id(case), 'v2' if v2 else 'v1', '  '.join('%s %.2e' % kv for kv in errs.items())))
    for name, err in errs.items():
        assert err < ORACLE_TOL, (name, err)


@pytest.mark.parametrize('v2', [False, True], ids=['v1', 'v2'])
@pytest.mark.parametrize('case', E.CASES, ids=E.case_id)
def test_all_outside_gives_exact_zeros_in_the_oracle(case, v2):
    for dtype in (np.float32, np.float64):
        r = E.reference(case, 'outside', v2, SEED, dtype)
        bias = r['bias']
        want_y = np.zeros_like(r['y']) if bias is None else np.broadcast_to(bias.astype(dtype).reshape(1, -1, 1, 1), r['y'].shape)
        assert np.array_equal(r['y'], want_y)
        for name in ('grad_input', 'grad_offset', 'grad_weight') + (('grad_mask',) if v2 else ()):
            assert not r[name].any(), name
