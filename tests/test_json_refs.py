"""``evaluation_device.json_restatement`` -- the reference of the result-file kernels (csrc/coco_json.hip) -- against
``evaluation.results2json`` / ``kpt2json`` + ``json.dump`` byte for byte, and its formatter rule against ``repr``.  No GPU."""
import io
import json
import os

import numpy as np
import pytest

from kgdet_amd import evaluation as ev
from kgdet_amd import evaluation_device as evd
from tests import json_cases as jc


def _host_files(c, tmp_path, rows=None, tag='host'):
    files = ev.results2json(c.dataset, jc.host_results(c, rows), str(tmp_path / tag))
    with open(files['bbox'], 'rb') as f:
        box = f.read()
    with open(files['keypoints'], 'rb') as f:
        kpt = f.read()
    return box, kpt


def _dumped(lists):
    out = []
    for records in lists:
        s = io.StringIO()
        json.dump(records, s)
        out.append(s.getvalue().encode('ascii'))
    return tuple(out)


@pytest.mark.parametrize('name', jc.NAMES)
def test_restatement_equals_results2json(name, tmp_path):
    c = jc.case(name)
    want = _host_files(c, tmp_path)
    got = evd.json_restatement(c.dataset, c.rows, 4, num_labels=c.n_labels)
    assert got[0] == want[0]
    assert got[1] == want[1]
    n = sum(len(part) for res in jc.host_results(c) for part in res[0])
    assert n > 0 and len(json.loads(got[0].decode())) == n and len(json.loads(got[1].decode())) == n


@pytest.mark.parametrize('num_digits', [1, 2, 3])
@pytest.mark.parametrize('name', ['k22', 'edge'])
def test_restatement_equals_kpt2json_at_fewer_digits(name, num_digits):
    c = jc.case(name)
    want = _dumped(ev.kpt2json(c.dataset, jc.host_results(c), num_digits))
    got = evd.json_restatement(c.dataset, c.rows, num_digits, num_labels=c.n_labels)
    assert got[0] == want[0]
    assert got[1] == want[1]


def test_the_edge_set_keeps_signed_zeros_and_integer_fractions():
    c = jc.case('edge')
    box, kpt = evd.json_restatement(c.dataset, c.rows, 4, num_labels=c.n_labels)
    for text in (b'-0.0,', b' 0.0,', b' 12.0,', b' 1.0,', b'-123.4567,', b' 1099511.5,', b' 109951160.0,', b' 0.0001,',
                 b'"image_id": 1099511627776,', b'"image_id": 0,'):
        assert text in kpt, text
    assert b'-2.25,' in box and b'e-' not in kpt and b'e-' not in box


@pytest.mark.parametrize('num_digits', [1, 2, 3, 4])
def test_formatter_rule_equals_repr(num_digits):
    v = jc.formatter_values(num_digits)
    assert len(v) > 19000
    wide = v.astype(np.float64)
    q, neg, bad = evd.decimals_of_landmarks(v, num_digits)
    assert bad == 0
    got = evd.format_decimals(q, neg, num_digits)
    want = [repr(float(np.round(np.float64(np.float32(x)), num_digits))) for x in v]
    assert got == want
    rounded = evd.round_half_even_restatement(wide, num_digits)
    got = evd.format_decimals(*evd.decimals_of_rounded(rounded, num_digits), num_digits)
    want = [repr(round(float(x), num_digits)) for x in wide]
    assert got == want


def test_an_empty_set_gives_empty_lists(tmp_path):
    c = jc.empty_case()
    assert evd.json_restatement(c.dataset, c.rows, 4) == (b'[]', b'[]')
    assert _host_files(c, tmp_path) == (b'[]', b'[]')
    none = jc.Case(dataset=jc.Dataset([], jc.CATS_13), rows=np.zeros((0, jc.M, 10), np.float32), n_labels=13)
    assert evd.json_restatement(none.dataset, none.rows, 4) == (b'[]', b'[]')


def test_what_the_restatement_refuses():
    c = jc.case('k1')
    for d in (0, 5, -1, 2.0, 4.0, True):
        with pytest.raises(ValueError):
            evd.json_restatement(c.dataset, c.rows, d)
    for value in jc.OUTSIDE:
        rows = c.rows.copy()
        rows[0, 2, 8] = value
        with pytest.raises(ValueError):
            evd.json_restatement(c.dataset, rows, 4)
    rows = c.rows.copy()
    rows[0, 2, 2] = 3e8                                             # (the width leaves the rounding's domain)
    with pytest.raises(ValueError):
        evd.json_restatement(c.dataset, rows, 4)
    rows = c.rows.copy()
    rows[3, 0, 6] = jc.M + 1
    with pytest.raises(ValueError):
        evd.json_restatement(c.dataset, rows, 4)
    with pytest.raises(ValueError):
        evd.json_restatement(c.dataset, c.rows, 4, num_labels=14)     # more labels than the dataset's categories
    for ids in ([0, 7, -1, 4, 5], [0, 7, 2 ** 63, 4, 5], [0, 7, 1.0, 4, 5], [0, 7, 'a', 4, 5]):
        with pytest.raises(ValueError):
            evd.json_restatement(jc.Dataset(ids, jc.CATS_13), c.rows, 4)
    with pytest.raises(ValueError):
        evd.json_restatement(jc.Dataset(jc.IMG_IDS, [-3] + jc.CATS_13[1:]), c.rows, 4)


class _HostRows(object):
    """a ``runner.DeviceResults`` whose rows lie on the CPU"""

    def __init__(self, c, rows=None):
        import torch
        from kgdet_amd.runner import DeviceResults
        self.dev = DeviceResults(torch.from_numpy((c.rows if rows is None else rows).copy()), c.n_labels + 1)


def test_rows_on_the_cpu_take_the_restatement_and_leave_the_same_files(tmp_path):
    c = jc.case('k22')
    want = _host_files(c, tmp_path)
    dev = _HostRows(c).dev
    files = evd.write_device_results_json(c.dataset, dev, str(tmp_path / 'dev'))
    assert files == {k: str(tmp_path / 'dev') + '.%s.json' % ('keypoints' if k == 'keypoints' else 'bbox')
                     for k in ('bbox', 'proposal', 'keypoints')}
    with open(files['bbox'], 'rb') as f:
        assert f.read() == want[0]
    with open(files['keypoints'], 'rb') as f:
        assert f.read() == want[1]
    assert sorted(os.listdir(str(tmp_path))) == ['dev.bbox.json', 'dev.keypoints.json', 'host.bbox.json', 'host.keypoints.json']
    evd.results2json_any(c.dataset, dev, str(tmp_path / 'any'))
    ev.results2json(c.dataset, dev.to_host(), str(tmp_path / 'list'))
    for kind in ('bbox', 'keypoints'):
        with open(str(tmp_path / ('any.%s.json' % kind)), 'rb') as f, open(str(tmp_path / ('list.%s.json' % kind)), 'rb') as g:
            assert f.read() == g.read()


def test_a_refused_set_leaves_no_file_and_results2json_any_takes_the_host_route(tmp_path):
    c = jc.case('k1')
    rows = c.rows.copy()
    rows[0, 2, 8] = np.inf
    dev = _HostRows(c, rows).dev
    with pytest.raises(ValueError):
        evd.write_device_results_json(c.dataset, dev, str(tmp_path / 'dev'))
    assert os.listdir(str(tmp_path)) == []
    with pytest.warns(RuntimeWarning) as seen:
        files = evd.results2json_any(c.dataset, dev, str(tmp_path / 'any'))
    seen = [w for w in seen if issubclass(w.category, RuntimeWarning)]
    assert len(seen) == 1 and 'not finite' in str(seen[0].message)
    want = _host_files(c, tmp_path, rows)
    with open(files['bbox'], 'rb') as f:
        assert f.read() == want[0]
    with open(files['keypoints'], 'rb') as f:
        assert f.read() == want[1]
    dev.release()
    with pytest.raises(ValueError):
        evd.write_device_results_json(c.dataset, dev, str(tmp_path / 'gone'))
    lists = jc.host_results(c)
    assert evd.results2json_any(c.dataset, lists, str(tmp_path / 'plain'))['keypoints'].endswith('plain.keypoints.json')
