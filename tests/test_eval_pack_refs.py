"""The numpy side of the device packing (kgdet_amd/evaluation_device.py): ``round_half_even_restatement`` against Python's
``round``, ``pack_rows_restatement`` against ``pack_test_results(..., lazy_landmarks=True)`` on the list form of the same
detections, ``DeviceResults.to_host()``, and ``evaluate_results`` on a ``DeviceResults`` whose rows lie on the CPU.  Equality of
bits throughout: the rounding is exact by construction, everything else is integers, copies and single float64 operations."""
import numpy as np
import pytest
import torch

from kgdet_amd import evaluation_device as evd
from kgdet_amd.runner import DeviceResults
from tests import eval_pack_cases as pack

INT_FIELDS = ('cell', 'start', 'img_idx', 'cat_idx', 'id')


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_packed(got, want, what):
    for kind in ('bbox', 'keypoints'):
        g, w = got[kind], want[kind]
        assert g.kind == w.kind == kind
        for f in INT_FIELDS:
            assert getattr(g, f).dtype == np.int64 and np.array_equal(getattr(g, f), getattr(w, f)), (what, kind, f)
        assert same_bits(g.score, w.score), (what, kind, 'score')
        assert g.kxy is None and w.kxy is None
    assert same_bits(got['bbox'].bbox, want['bbox'].bbox) and same_bits(got['bbox'].area, want['bbox'].area), what
    gk, wk = got['keypoints'], want['keypoints']
    assert gk.bbox is None and wk.bbox is None and gk.area is None and wk.area is None and gk.num_digits == wk.num_digits
    kxy = gk.kxy32 if isinstance(gk.kxy32, np.ndarray) else gk.kxy32.cpu().numpy()
    assert same_bits(kxy, wk.kxy32), (what, 'kxy32')


@pytest.mark.parametrize('d', [1, 4, 9])
def test_rounding_restatement_is_pythons_round(d):
    v = pack.rounding_inputs(d)
    assert len(v) >= 200000 + len(pack.rounding_pool()) and (np.abs(v) * 10.0 ** d < evd.ROUND_LIMIT).all()
    got = evd.round_half_even_restatement(v, d)
    want = np.array([round(float(x), d) for x in v])
    bad = np.nonzero(got.view(np.int64) != want.view(np.int64))[0]           # (bit patterns: the sign of a zero counts)
    assert len(bad) == 0, (d, v[bad[:5]], got[bad[:5]], want[bad[:5]])


def test_rounding_restatement_leaves_what_it_cannot_round():
    v = np.array([np.inf, -np.inf, np.nan, 2e8, 1.0])
    out, n_bad = evd._round_half_even(v, 4)
    assert n_bad == 4 and out[4] == 1.0 and out[3] == 2e8 and np.isinf(out[:2]).all() and np.isnan(out[2])


@pytest.mark.parametrize('name', pack.NAMES)
def test_rows_restatement_equals_the_host_packing(name):
    c = pack.case(name)
    pg = pack.packed_gt(c)
    want = evd.pack_test_results(pg, c.dataset, c.results, 4, lazy_landmarks=True)
    got = evd.pack_rows_restatement(pg, c.dataset, c.rows, 4)
    assert_same_packed(got, want, name)
    if name == 'cuts':
        assert np.diff(got['bbox'].start).max() == 100 and np.diff(got['keypoints'].start).max() == 20
    if name == 'empty':
        assert len(got['bbox'].score) == 0 and got['keypoints'].kxy32.shape == (0, 3 * c.K)
    if name != 'empty':
        ids = got['bbox'].id
        assert ids.max() > len(ids) or name in ('single', 'ties'), 'rows of the unknown label count in the ids'


@pytest.mark.parametrize('name', pack.NAMES)
def test_to_host_is_the_list_the_rows_were_made_from(name):
    c = pack.case(name)
    got = DeviceResults(torch.from_numpy(c.rows), c.n_labels + 1).to_host()
    assert len(got) == len(c.results)
    for g, w in zip(got, c.results):
        assert type(g) is tuple and len(g) == len(w)
        for part_g, part_w in zip(g, w):
            parts = zip(part_g, part_w) if isinstance(part_w, list) else [(part_g, part_w)]
            for x, y in parts:
                assert same_bits(x, y)


def test_device_results_release():
    c = pack.case('ties')
    dev = DeviceResults(torch.from_numpy(c.rows), c.n_labels + 1)
    assert len(dev) == 2
    dev.release()
    assert dev.rows is None
    with pytest.raises(ValueError):
        dev.to_host()


def test_unknown_image_with_detections_is_refused():
    c = pack.case('ties')
    pg = pack.packed_gt(c)
    other = pack.Dataset(c.dataset.coco, [12345] + c.dataset.img_ids[1:], c.dataset.cat_ids)
    with pytest.raises(ValueError):
        evd.pack_rows_restatement(pg, other, c.rows, 4)
    with pytest.raises(ValueError):
        evd.pack_test_results(pg, other, c.results, 4, lazy_landmarks=True)
    for d in (True, 4.0):                                           # (num_digits is an int, as for the result files)
        with pytest.raises(ValueError):
            evd.pack_rows_restatement(pg, c.dataset, c.rows, d)


@pytest.mark.parametrize('bad', [np.inf, 2e8])
def test_values_outside_the_rounding_domain_are_refused(bad):
    c = pack.case('ties')
    rows = c.rows.copy()
    rows[0, 1, 4 if np.isinf(bad) else 0] = bad
    with pytest.raises(ValueError):
        evd.pack_rows_restatement(pack.packed_gt(c), c.dataset, rows, 4)


def test_evaluate_results_on_cpu_rows_equals_the_list_route():
    c = pack.case('mixed')
    pg = pack.packed_gt(c)
    want = evd.evaluate_results(c.dataset, c.results, device='cpu', packed_gt=pg)
    dev = DeviceResults(torch.from_numpy(c.rows), c.n_labels + 1)
    got = evd.evaluate_results(c.dataset, dev, device='cpu', packed_gt=pg)
    assert dev.rows is None
    for t in ('bbox', 'keypoints'):
        assert np.array_equal(got[t], want[t]), t
    assert want['bbox'][0] > 0.05 and want['keypoints'][0] > 0.05       # (the case scores something)


def test_runner_refuses_device_results_with_a_process_group():
    from kgdet_amd import runner as rn
    ok = rn.Runner(None, None, logger=lambda s: None, eval_config=dict(dataset=None, device_results=True))
    assert ok.eval_config['device_results'] is True
    with pytest.raises(ValueError):
        rn.Runner(None, None, logger=lambda s: None, eval_config=dict(dataset=None, device_results=True, group=object()))
