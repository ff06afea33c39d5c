"""tests/eval_kernel_cases.py held to its own claims on the CPU: the scalar references agree with the numpy restatements that
sit next to the kernels (``evaluation_device.similarity_restatement`` / ``match_restatement``) on every case, the scalar matcher
reproduces ``CocoEvaluator`` on a golden detection set, and each case contains the decisions it is named for."""
import numpy as np
import pytest

from kgdet_amd import evaluation_device as evd
from tests import eval_cases
from tests import eval_kernel_cases as E


def _sim_in_domain(c):
    """the cells ``similarity_restatement`` may index: the ones the kernels take"""
    import types
    keep = [i for i, (cell, off) in enumerate(zip(c.cells, c.sim_off))
            if E.cell_valid(cell, c.nd, c.ng) and (E.sim_valid(cell, int(off), c.sim_size) or cell[1] == 0 or cell[3] == 0)]
    out = types.SimpleNamespace(**vars(c))
    out.cells, out.sim_off = c.cells[keep], c.sim_off[keep]
    return out


@pytest.mark.parametrize('name', E.SIM_NAMES)
def test_similarity_reference_and_restatement_agree(name):
    c = E.sim_case(name)
    want = E.reference_similarity(c)
    written = ~(want.view(np.uint64) == np.array([E.FILL_SIM]).view(np.uint64)[0])
    theirs = evd.similarity_restatement(_sim_in_domain(c))
    assert written.any() and not written.all()                        # (the reserved words of the skipped cells keep the fill)
    assert np.array_equal(want[written], theirs[written])
    assert (theirs[~written] == 0).all()
    kinds = dict(valid=0, skipped=0, no_sim=0, empty=0)
    for cell, off in zip(c.cells, c.sim_off):
        if not E.cell_valid(cell, c.nd, c.ng):
            kinds['skipped'] += 1
        elif cell[1] == 0 or cell[3] == 0:
            kinds['empty'] += 1
        elif E.sim_valid(cell, int(off), c.sim_size):
            kinds['valid'] += 1
        else:
            kinds['no_sim'] += 1
    assert kinds['skipped'] == 4 and kinds['no_sim'] == 2 and kinds['empty'] == 3 and kinds['valid'] >= 3, kinds
    assert sorted(int(o + cell[1] * cell[3]) for cell, o in zip(c.cells, c.sim_off))[-1] == c.sim_size + 1
    assert -1 in c.sim_off
    assert not np.array_equal(c.sim_off[c.sim_off >= 0], np.sort(c.sim_off[c.sim_off >= 0]))          # listed out of array order
    sizes = {int(cell[1]) * int(cell[3]) for cell, off in zip(c.cells, c.sim_off) if E.cell_valid(cell, c.nd, c.ng)}
    assert 1 in sizes and 0 in sizes
    if name in ('iou', 'oks1', 'oks65'):
        assert 70 * 33 in sizes


def test_iou_case_contains_its_edges():
    c = E.iou_case()
    sim = E.reference_similarity(c)
    d0, D, g0, G = c.cells[[tuple(x) for x in c.cells].index((0, 9, 0, 9))]
    off = int(c.sim_off[[tuple(x) for x in c.cells].index((0, 9, 0, 9))])
    block = sim[off:off + D * G].reshape(D, G)
    assert block[0, 0] == 1.0 and block[6, 3] == 1.0 and block[7, 6] == 1.0          # identical boxes: exactly 1
    assert block[0, 1] == 0.0 and block[0, 2] == 0.0                                  # touching: iw == 0 / ih == 0
    assert (block[2:6] == 0.0).all()                                                  # zero and negative extents
    assert 0.0 < block[8, 6] < 1.0                                                    # coordinates at 1e8
    assert block[0, 7] == 1.0 and 0.0 < block[0, 8] < 0.1                             # inside a crowd: its own area is the union
    crowd = [tuple(x) for x in c.cells].index((9, 4, 9, 2))
    b2 = sim[int(c.sim_off[crowd]):int(c.sim_off[crowd]) + 8].reshape(4, 2)
    assert (b2[:3] == 0.0).all() and b2[3, 0] == 1.0                                  # zero-area detections against a crowd: 0, no 0 / 0
    assert np.isfinite(sim[~np.isnan(sim)]).all() and not np.isnan(block).any()


@pytest.mark.parametrize('K', E.SIM_KS)
def test_oks_cases_contain_their_edges(K):
    c = E.oks_case(K)
    sim = E.reference_similarity(c)
    n_one = n_zero = 0
    for off, ones, zeros, risky in E.oks_arguments(c):
        assert risky == 0, 'an exponent argument inside (690, 746]: re-draw the case'
        block = sim[off:off + ones.size].reshape(ones.shape)
        assert (block[ones] == 1.0).all() and (block[zeros] == 0.0).all()
        n_one += int(ones.sum()); n_zero += int(zeros.sum())
        rest = block[~ones & ~zeros]
        assert ((rest > 0) & (rest < 1)).all()
    assert n_one >= 4 and n_zero >= 3
    assert (c.g_nvis == 0).any() and (c.g_area == 0).any()
    assert {-1.0, 0.0, 1.0, 2.0} <= set(np.unique(c.g_kpt[:, 2::3])) or K == 1
    values = sim[~np.isnan(sim)]
    assert ((values == 0) | (values > 1e-280)).all()


# --- matching ------------------------------------------------------------------------------------------------------------------
def _lanes(c, name):
    d0, D, g0, G = E.cell_of(c, name)
    dm, di, gi = E.reference_match(c)
    return dm[d0:d0 + D], di[d0:d0 + D], gi[g0:g0 + G], g0


@pytest.mark.parametrize('A,T', E.MATCH_SHAPES)
def test_match_reference_and_restatement_agree(A, T):
    c = E.match_case(A, T)
    assert c.area_rng.shape == (A, 2) and c.best0.shape == (T, ) and (np.diff(c.best0) > 0).all()
    want = E.reference_match(c)
    dom, sim = E.in_domain(c, c.sim)
    theirs = evd.match_restatement(dom, sim)
    rows_d, rows_g = E.written_rows(c)
    assert rows_d.any() and not rows_d.all() and rows_g.any() and not rows_g.all()
    assert np.array_equal(want[0][rows_d], theirs[0][rows_d])
    assert np.array_equal(want[1][rows_d], theirs[1][rows_d])
    assert np.array_equal(want[2][rows_g], theirs[2][rows_g])
    assert (want[0][~rows_d] == E.FILL_I32).all() and (want[1][~rows_d] == E.FILL_U8).all() and (want[2][~rows_g] == E.FILL_U8).all()
    assert not (want[0][rows_d] == E.FILL_I32).any() and not (want[1][rows_d] == E.FILL_U8).any()


@pytest.mark.parametrize('A,T', E.MATCH_SHAPES)
def test_match_case_contains_its_decisions(A, T):
    c = E.match_case(A, T)
    tq = c.tq
    # a similarity exactly on the threshold matches, one float below does not; 1.0 matches under every threshold (cap 1 - 1e-10)
    dm, di, gi, g0 = _lanes(c, 'threshold')
    assert (dm[0, 0, :tq + 1] == g0 + 1).all() and (dm[0, 0, tq + 1:] == 0).all()
    assert (dm[1, 0, :tq] == g0 + 2).all() and (dm[1, 0, tq:] == 0).all()
    assert (dm[2, 0, :] == g0 + 3).all()
    if c.thr[-1] == 1.0:
        assert c.best0[-1] == 1 - 1e-10 < 1.0
    # equal candidates: the later one wins, the earlier one is left for the next detection
    dm, di, gi, g0 = _lanes(c, 'ties')
    lane = c.best0 <= 0.75
    assert lane.any() and (dm[0, 0, lane] == g0 + 2).all() and (dm[1, 0, lane] == g0 + 1).all() and (dm[2, 0, lane] == 0).all()
    dm3, _, _, g3 = _lanes(c, 'ties3')
    lane = c.best0 <= 0.875
    assert (dm3[0, 0, lane] == g3 + 3).all() and (dm3[1, 0, lane] == g3 + 1).all()
    # an ignored ground truth with the higher similarity, listed first: the regular one wins where it passes
    dm, di, gi, g0 = _lanes(c, 'ignored_first')
    low, mid = c.best0 <= 0.625, (c.best0 > 0.75) & (c.best0 <= 0.875)
    if low.any():
        assert (dm[0, 0, low] == g0 + 3).all() and (di[0, 0, low] == 0).all()         # (area range 'all': slot 2 at 0.75, regular)
    if mid.any():
        assert (dm[0, 0, mid] == g0 + 1).all() and (di[0, 0, mid] == 1).all()         # only the ignored one passes
    assert list(gi[:, 0]) == [1, 0, 0, 0]
    if A > 1:
        assert len({tuple(row) for row in gi[1:]}) > 1                                 # regular in one area range, ignored in another
    # areas exactly on the borders are inside
    _, _, gi, _ = _lanes(c, 'gt_areas_on_borders')
    dmb, dib, _, _ = _lanes(c, 'det_areas_on_borders')
    assert (dmb == 0).all()
    if A in (3, 4):
        medium = 1 if A == 3 else 2
        assert list(gi[:, medium]) == [0, 0, 1, 1, 1, 1] and list(dib[:, medium, 0]) == [0, 0, 1, 1, 1, 1, 1]
        assert list(gi[:, 0]) == [0] * 6 and list(dib[:, 0, 0]) == [0] * 6 + [1]
    # a crowd takes every detection, a regular ground truth one
    dm, di, gi, g0 = _lanes(c, 'crowd_reused')
    lane = c.best0 <= 0.75
    assert (dm[:3, 0][:, lane] == g0 + 1).all() and (di[:3, 0][:, lane] == 1).all() and (dm[3, 0, lane] == g0 + 2).all()
    dm, _, _, g0 = _lanes(c, 'regular_once')
    lane = c.best0 <= 0.96875
    assert (dm[0, 0, lane] == g0 + 1).all() and (dm[1, 0, lane] == 0).all() and (dm[2, 0, ~lane] == g0 + 1).all()
    dm, _, _, g0 = _lanes(c, 'ignored_not_crowd_once')
    lane = c.best0 <= 0.875
    assert (dm[0, 0, lane] == g0 + 1).all() and (dm[1, 0, lane] == 0).all()
    # degenerate cells
    dm, di, gi, _ = _lanes(c, 'no_ground_truth')
    assert (dm == 0).all() and gi.shape[0] == 0
    dm, di, gi, _ = _lanes(c, 'no_detection')
    assert dm.shape[0] == 0 and list(gi[:, 0]) == [0, 0, 1, 0]
    for name in ('sim_off_negative', 'sim_off_past_the_end'):
        dm, di, gi, _ = _lanes(c, name)
        assert (dm == 0).all() and (gi != E.FILL_U8).all() and (di != E.FILL_U8).all()
    dm, _, _, g0 = _lanes(c, 'nan_similarity')
    assert (dm[0] == g0 + 3).all()                                    # NaN < best is false: accepted, and so is what follows
    for name in ('skipped_negative_start', 'skipped_past_NG', 'skipped_past_ND'):
        assert not E.cell_valid(E.cell_of(c, name), c.nd, c.ng)
    offs = dict(zip(c.cell_names, c.sim_off))
    d0, D, g0, G = E.cell_of(c, 'sim_off_past_the_end')
    assert offs['sim_off_past_the_end'] + D * G == c.sim_size + 1 and offs['sim_off_negative'] == -1


def test_scalar_matcher_reproduces_the_coco_evaluator_on_a_golden_case():
    """case 'a' of tests/eval_cases.py, both result types: the scalar loop on the packed chunk in place of the restatement gives
    CocoEvaluator's eval_imgs entry by entry"""
    gt, results = eval_cases.golden_case('a')
    for typ in ('bbox', 'keypoints'):
        got = eval_cases.packed_evaluator(gt, results[typ], typ, 'cpu')
        want = eval_cases.host_evaluator(gt, results[typ], typ)
        chunks = list(got._chunks(1 << 30))
        assert len(chunks) == 1 and chunks[0].d0 == 0 and chunks[0].g0 == 0
        c = chunks[0]
        sim = evd.similarity_restatement(c)
        dm, di, gi = E.reference_match(c, sim)
        assert not (dm == E.FILL_I32).any() and not (gi == E.FILL_U8).any()
        theirs = evd.match_restatement(c, sim)
        assert np.array_equal(dm, theirs[0]) and np.array_equal(di, theirs[1]) and np.array_equal(gi, theirs[2])
        got._out = evd.Packed(d_match=dm, d_ignore=di.view(bool), g_ignore=gi, sim=sim, sim_start=got._out.sim_start)
        p = want.params
        Kc, A, I = len(p.cat_ids), len(p.area_rng), len(p.img_ids)
        n = 0
        for k in range(Kc):
            for a in range(A):
                for i in range(I):
                    w, g = want.eval_imgs[(k * A + a) * I + i], got.eval_imgs_of(k, a, i)
                    assert (w is None) == (g is None)
                    if w is None:
                        continue
                    n += 1
                    for key in ('d_match', 'g_ignore', 'd_ignore'):
                        assert w[key].shape == g[key].shape and np.array_equal(w[key], g[key]), (typ, key, k, a, i)
        assert n > 0
