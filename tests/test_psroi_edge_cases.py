"""tests/psroi_edge_cases.py held to its own claims on the CPU, before a GPU is involved: the table reaches the launcher paths it
names, the exact family's positions are the same numbers in float32 and float64 and hit every class of the sampling rule, the two
oracles agree on `count` in every bin of every case, and the float64 oracle agrees with the independent grid_sample formulation of
tests/torch_ref.py where tests/test_oracle_dcn.py never goes (P != 7, part_size > P, group_size > P, P = 1, 1 x 1 maps)."""
import functools

import numpy as np
import pytest

from tests import psroi_edge_cases as E

EXACT = [c for c in E.CASES if c.family == 'exact']
GENERAL = [c for c in E.CASES if c.family == 'general']
HANDOVER = E.BY_NAME['handover']


def _pow2(v):
    return v > 0 and np.log2(v) == np.floor(np.log2(v))


def test_the_table_reaches_the_paths_it_names():
    per_class = lambda c: c.out_dim // E.classes_of(c)
    nrec = lambda c: c.pooled_size ** 2 * c.sample_per_part ** 2
    for c in E.CASES:
        # inside the envelope of psroi_check
        assert c.out_dim * c.group_size ** 2 <= c.C and c.out_dim % E.classes_of(c) == 0
        assert nrec(c) <= 2048 and c.pooled_size <= 16 and c.group_size <= 16 and 0.0 <= c.trans_std <= 1.0
    some = lambda pred: any(pred(c) for c in E.CASES)
    assert some(lambda c: per_class(c) % 4 == 0) and some(lambda c: per_class(c) % 4 != 0)          # lists<4>, lists<1>
    assert some(lambda c: per_class(c) > 64 and per_class(c) % 64 != 0 and per_class(c) % 4 != 0)   # chunk tails, lists<1> x 2
    assert some(lambda c: per_class(c) > 256 and per_class(c) % 256 != 0 and per_class(c) % 4 == 0)  # lists<4> x 2 chunks
    assert some(lambda c: c.out_dim > 128 and c.out_dim % 64 != 0)                                  # three channel tiles, a tail
    assert some(lambda c: c.C > c.out_dim * c.group_size ** 2)
    assert some(lambda c: nrec(c) <= 256) and some(lambda c: 256 < nrec(c) <= 832) and some(lambda c: nrec(c) > 832)
    assert some(lambda c: c.pooled_size ** 2 == 256) and some(lambda c: 64 < c.pooled_size ** 2 < 128)
    assert {2025, 1936, 1024} <= {nrec(c) for c in E.CASES}
    assert some(lambda c: c.sample_per_part ** 2 % 4 == 1 and c.sample_per_part > 1) and some(lambda c: c.sample_per_part == 1)
    assert some(lambda c: c.part_size > c.pooled_size and E.empty_offset_cells(c).any())
    assert some(lambda c: c.group_size > c.pooled_size and E.empty_group_channels(c)[:c.out_dim * c.group_size ** 2].any())
    assert some(lambda c: per_class(c) == 1 and E.classes_of(c) == 3 and c.group_size == 1)
    assert some(lambda c: c.H == 1 and c.W == 1) and some(lambda c: c.W == 2) and some(lambda c: c.H * c.W % 64 and c.H * c.W > 64)
    assert some(lambda c: c.family == 'exact' and c.trans_std == 0.0 and not c.no_trans)
    assert some(lambda c: c.trans_std == 1.0) and some(lambda c: c.family == 'exact' and c.no_trans)
    assert some(lambda c: c.family == 'general' and c.no_trans)
    assert HANDOVER.R == 20101 and HANDOVER.R > 4 * 4096


@pytest.mark.parametrize('case', E.CASES, ids=E.case_id)
def test_inputs_are_fixed_float32_and_shaped(case):
    a, b = E.inputs(case), E.inputs(case)
    c = case
    want = dict(data=(c.B, c.C, c.H, c.W), rois=(c.R, 5), grad_out=(c.R, c.out_dim, c.pooled_size, c.pooled_size),
                offset=(c.R, 2 * c.num_classes, c.part_size, c.part_size))
    for name, shape in want.items():
        if name == 'offset' and c.no_trans:
            assert a[name] is None
            continue
        assert a[name].dtype == np.float32 and a[name].shape == shape and np.isfinite(a[name]).all()
        assert a[name].tobytes() == b[name].tobytes()


@pytest.mark.parametrize('case', EXACT, ids=E.case_id)
def test_exact_family_is_built_from_dyadic_numbers(case):
    inp = E.inputs(case)
    rois = inp['rois'].astype(np.float64)
    assert _pow2(case.pooled_size) and _pow2(case.sample_per_part)
    assert case.trans_std == 0.0 or _pow2(case.trans_std)
    assert np.array_equal(rois, np.round(rois))
    assert not ((rois[:, 3] + 1 - rois[:, 1]) % 16).any() and not ((rois[:, 4] + 1 - rois[:, 2]) % 16).any()
    assert (rois[:, 3] >= rois[:, 1]).all() and (rois[:, 4] >= rois[:, 2]).all()
    if not case.no_trans:
        o8 = inp['offset'].astype(np.float64) * 8
        assert np.array_equal(o8, np.round(o8))


@pytest.mark.parametrize('case', EXACT + [HANDOVER], ids=E.case_id)
def test_exact_float32_positions_equal_float64_positions_bit_for_bit(case):
    inp = E.inputs(case)
    p32 = E.positions(case, inp['rois'], inp['offset'], np.float32)
    p64 = E.positions(case, inp['rois'], inp['offset'], np.float64)
    for a32, a64 in zip(p32, p64):
        assert a32.dtype == np.float32 and a64.dtype == np.float64
        assert np.array_equal(a32.astype(np.float64), a64)


@pytest.mark.parametrize('case', EXACT, ids=E.case_id)
def test_every_class_of_position_is_hit_in_both_axes(case):
    """The two hair positions need an offset step of 2^-10 of a map cell: the exact cases without one (no_trans, trans_std 0 or 1)
    have coordinates that are multiples of 1/16 at the finest and cannot produce them; they must produce every other class."""
    inp = E.inputs(case)
    counts = E.classify(case, inp['rois'], inp['offset'])
    possible = E.possible_classes(case)
    assert possible == set(E.CLASSES) or (possible == set(E.CLASSES) - {'hair_lo', 'hair_hi'} and not E.fine_offsets(case))
    assert E.fine_offsets(case) == (not case.no_trans and case.trans_std == E.T7)
    print(case.name, counts)
    for axis in ('x', 'y'):
        for cls in E.CLASSES:
            if cls in possible:
                assert counts[axis][cls] > 0, (axis, cls, counts[axis])
            else:
                assert counts[axis][cls] == 0, (axis, cls)


@pytest.mark.parametrize('case', E.CASES, ids=E.case_id)
def test_bins_empty_partial_and_identical_in_both_oracles(case):
    """count: float32 oracle == float64 oracle == the positions of E.positions, in EVERY bin; at most half of the bins empty; at
    least 3 % partially clipped -- where a bin has more than one sample (0 < count < 1 does not exist)."""
    r = E.reference(case)
    SS = case.sample_per_part ** 2
    assert r['count'].dtype == np.float64 and r['count32'].dtype == np.float32
    assert np.array_equal(r['count'], r['count32'].astype(np.float64))
    for dtype in (np.float32, np.float64):      # the bin -> offset cell / group cell maps do not depend on the precision either
        assert all(np.array_equal(a, b) for a, b in zip(E.bin_maps(case, dtype), E.bin_maps(case, np.float64)))
    ok = E.valid_rows(case, r['rois'])
    w, h = E.positions(case, r['rois'][ok], None if case.no_trans else r['offset'][ok])
    mine = E.sample_alive(case, w, h).sum((-1, -2))                                  # [R, classes, P, P]
    per_class = case.out_dim // E.classes_of(case)
    assert np.array_equal(np.repeat(mine, per_class, axis=1), r['count'][ok])
    cnt = r['count'][ok]
    empty, partial = float((cnt == 0).mean()), float(((cnt > 0) & (cnt < SS)).mean())
    print('%s: empty %.3f partial %.3f' % (case.name, empty, partial))
    assert empty <= 0.5
    assert partial >= 0.03 if SS > 1 else partial == 0.0
    assert not r['out'][~ok].any() and not r['count'][~ok].any()
    if not case.no_trans:
        assert not r['grad_trans'][~ok].any()


@pytest.mark.parametrize('case', GENERAL, ids=E.case_id)
def test_general_family_has_the_whole_map_and_a_zero_width_roi(case):
    rois = E.inputs(case)['rois']
    lo, ext, _, _ = E.geometry(case, rois)
    assert np.allclose(lo[0], -0.5) and np.allclose(ext[0], [case.W, case.H])
    assert np.array_equal(ext[1], [0.1, 0.1])                       # 1/16 < 0.1: the fmax branch
    assert np.array_equal(E.geometry(case, rois, np.float32)[1][1], np.float32([0.1, 0.1]))


def test_handover_lists_have_exactly_the_lengths_at_the_sort_boundaries():
    inp = E.inputs(HANDOVER)
    n = E.list_lengths(HANDOVER, inp['rois'], None)
    assert n.shape == (10, 1, 1, 3, 3)
    for b, k in enumerate(E.HANDOVER_LENGTHS):
        want = np.zeros((3, 3), np.int64)
        want[:2, :2] = k
        assert np.array_equal(n[b, 0, 0], want)
    w, h = E.positions(HANDOVER, inp['rois'], None)
    assert (w == 0.75).all() and (h == 0.25).all()
    go = inp['grad_out']
    assert len(np.unique(go[:, 0, 0, 0])) > 0.99 * HANDOVER.R   # random per RoI: another order changes the float32 sum


def test_rois_outside_the_batch_and_images_without_rois():
    case = E.BY_NAME['noroi']
    r = E.reference(case)
    b = r['rois'][:, 0]
    assert b[2] == -1 and b[3] == case.B and (np.delete(b, [2, 3]) == 1).all()
    assert not r['grad_data'][0].any() and not r['grad_data'][2].any() and r['grad_data'][1].any()
    assert r['out'][4:].any() and r['count'][4:].any()


@pytest.mark.parametrize('case', [c for c in E.CASES if E.empty_offset_cells(c).any() or E.empty_group_channels(c).any()],
                         ids=E.case_id)
def test_cells_that_own_no_bin_have_zero_gradient_in_the_oracle(case):
    r = E.reference(case)
    dead = E.empty_group_channels(case)
    assert not r['grad_data'][:, dead].any() and not r['grad_data32'][:, dead].any()
    assert r['grad_data'][:, ~dead].any()
    if not case.no_trans:
        cells = E.empty_offset_cells(case)
        assert not r['grad_trans'][:, :, cells].any() and not r['grad_trans32'][:, :, cells].any()
        if case.trans_std > 0:
            assert r['grad_trans'][:, :, ~cells].any()


def test_trans_std_zero_ignores_the_offsets():
    r = E.reference(E.BY_NAME['tstd0'])
    assert r['offset'].any() and not r['grad_trans'].any() and not r['grad_trans32'].any()


TORCH_CASES = [c for c in E.CASES if c.family != 'handover']


@functools.lru_cache(maxsize=None)
def _compare_with_torch_ref(case):
    """Forward, count and grad_data of every case but the 20 101-RoI one against tests/torch_ref.deform_psroi_pool and its
    autograd in float64.  grad_trans: the kernel takes the slope between the floor and the ceil corner (zero on the lattice, not
    zero inside a clamp zone), autograd of a clamped coordinate differs at exactly those samples, so it is compared for the (RoI,
    class) blocks of the general family in which no alive sample lies in a clamp zone (test_oracle_dcn.py does the same)."""
    import torch
    from tests import torch_ref
    r = E.reference(case)
    c = case
    ok = E.valid_rows(c, r['rois'])
    f64 = lambda a: torch.from_numpy(a[ok].astype(np.float64))
    td = torch.from_numpy(r['data'].astype(np.float64)).requires_grad_()
    to = None if c.no_trans else f64(r['offset']).requires_grad_()
    out, cnt = torch_ref.deform_psroi_pool(td, f64(r['rois']), to, E.SCALE, c.pooled_size, c.out_dim, c.no_trans, c.group_size,
                                           c.part_size, c.sample_per_part, c.trans_std)
    assert np.array_equal(cnt.numpy(), r['count'][ok])
    np.testing.assert_allclose(out.detach().numpy(), r['out'][ok], rtol=0, atol=1e-12)
    out.backward(f64(r['grad_out']))
    np.testing.assert_allclose(td.grad.numpy(), r['grad_data'], rtol=0, atol=1e-11)
    if c.no_trans or c.family != 'general':
        return 0
    w, h = E.positions(c, r['rois'][ok], r['offset'][ok])
    alive = E.sample_alive(c, w, h)
    zone = lambda p, L: ((p >= -0.5) & (p < 0)) | ((p > L - 1) & (p <= L - 0.5))
    clamped = alive & (zone(h, c.H)[..., :, None] | zone(w, c.W)[..., None, :])
    free = ~clamped.any((-1, -2, -3, -4)) & alive.any((-1, -2, -3, -4))                 # [R, classes]
    got = to.grad.numpy().reshape(free.shape + (2, c.part_size, c.part_size))
    want = r['grad_trans'][ok].reshape(got.shape)
    np.testing.assert_allclose(got[free], want[free], rtol=0, atol=1e-10)
    return int(free.sum())


@pytest.mark.parametrize('case', TORCH_CASES, ids=E.case_id)
def test_float64_oracle_agrees_with_the_independent_formulation(case):
    _compare_with_torch_ref(case)


def test_the_offset_gradient_was_compared_in_enough_places():
    blocks = {c.name: _compare_with_torch_ref(c) for c in TORCH_CASES if c.family == 'general' and not c.no_trans}
    print(blocks)
    assert sum(blocks.values()) >= 10 and sum(v > 0 for v in blocks.values()) >= 4, blocks
