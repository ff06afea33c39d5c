"""``kgdet_coco_json_measure`` / ``kgdet_coco_json_write`` (csrc/coco_json.hip) through the C ABI, and the route they serve:
``single_gpu_test(..., device_results=True)`` -> ``write_device_results_json`` -> ``P.bbox.json`` / ``P.keypoints.json``.

The bar is EQUALITY of bytes with ``evaluation_device.json_restatement`` (held to ``evaluation.results2json`` on the CPU by
tests/test_json_refs.py) and, for the routes, with the files ``results2json`` writes.  Output buffers are pre-filled with 0xAA
between 64-byte canaries: every byte of a range must be written and nothing beside it."""
import ctypes
import filecmp
import importlib.util
import os
import warnings

import numpy as np
import pytest
import torch

from kgdet_amd import _lib
from kgdet_amd import evaluation as ev
from kgdet_amd import evaluation_device as evd
from kgdet_amd.checkpoint import save_checkpoint
from kgdet_amd.runner import DeviceResults, single_gpu_test
from tests import eval_pack_cases as pack
from tests import json_cases as jc
from tests import loader_cases as lc
from tests.golden import demo_cases
from tests.test_eval_pack_refs import assert_same_packed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
FILL, CANARY, PAD, SLACK = 0xAA, 0x5C, 64, 32
KINDS = ('bbox', 'keypoints')


class Measured(object):
    """kgdet_coco_order_dets (identity tables) + kgdet_coco_json_measure on a case through the C ABI, and the offsets scanned
    from the lengths as ``write_device_results_json`` scans them"""

    def __init__(self, c, rows=None, num_digits=4):
        rows = c.rows if rows is None else rows
        self.N, self.M, self.W = N, M, W = rows.shape
        self.L, self.d, self.cap = L, d, cap = c.n_labels, num_digits, N * M
        p, lib = _lib.ptr, _lib.lib()
        self.rows = torch.from_numpy(rows).cuda()
        self.img = torch.tensor(c.dataset.img_ids, dtype=torch.int64, device='cuda')
        self.cat = torch.tensor(c.dataset.cat_ids[:L], dtype=torch.int64, device='cuda')
        slot, col = torch.arange(N, dtype=torch.int32, device='cuda'), torch.arange(L, dtype=torch.int32, device='cuda')
        self.vals = torch.empty((N, M, 6), dtype=torch.float64, device='cuda')
        info = torch.empty((N, M, 3), dtype=torch.int32, device='cuda')
        img_rows = torch.empty(N, dtype=torch.int32, device='cuda')
        cnt = torch.empty((2, N * L), dtype=torch.int32, device='cuda')
        order_flags = torch.zeros(2, dtype=torch.int32, device='cuda')
        self.flags = torch.zeros(2, dtype=torch.int32, device='cuda')
        rc = lib.kgdet_coco_order_dets(p(self.rows), i64(N), i32(M), i32(W), p(slot), p(col), i32(L), i32(L), i64(N * L), i32(d),
                                       i32(100), i32(20), p(self.vals), p(info), p(img_rows), p(cnt[0]), p(cnt[1]),
                                       p(order_flags), _lib.current_stream())
        assert rc == 0, lib.kgdet_last_error()
        img_base = torch.cumsum(img_rows, dim=0, dtype=torch.int64) - img_rows
        self.lens = torch.zeros((2, cap), dtype=torch.int32, device='cuda')
        self.rec_src = torch.full((cap,), -1, dtype=torch.int64, device='cuda')
        rc = lib.kgdet_coco_json_measure(p(self.rows), i64(N), i32(M), i32(W), p(self.vals), p(info), p(img_base), p(self.img),
                                         p(self.cat), i32(L), i32(d), p(self.lens[0]), p(self.lens[1]), p(self.rec_src), i64(cap),
                                         p(self.flags), _lib.current_stream())
        assert rc == 0, lib.kgdet_last_error()
        self.R = int(img_rows.sum())
        self.offset = torch.zeros((2, cap + 1), dtype=torch.int64, device='cuda')
        self.offset[:, 1:] = torch.cumsum(self.lens, dim=1, dtype=torch.int64) + 2 * torch.arange(cap, dtype=torch.int64, device='cuda')
        self.off = self.offset.cpu().numpy()
        self.order_flags = order_flags.cpu().numpy()

    def write(self, kind, r0, r1, shift=0, override=()):
        """records [r0, r1) of a kind into a guarded buffer whose address is ``shift`` mod 16 -> (status, the range's bytes);
        asserts that nothing outside the range changed"""
        nbytes = int(self.off[kind, r1] - self.off[kind, r0]) if 0 <= r0 <= r1 else 0
        start = PAD + shift
        buf = torch.full((start + nbytes + SLACK + PAD,), CANARY, dtype=torch.uint8, device='cuda')
        buf[start:start + nbytes + SLACK] = FILL
        assert buf.data_ptr() % 16 == 0
        p = _lib.ptr
        a = dict(kind=kind, rows=p(self.rows), N=self.N, M=self.M, W=self.W, vals=p(self.vals), rec_src=p(self.rec_src),
                 offset=p(self.offset[kind]), img=p(self.img), cat=p(self.cat), L=self.L, d=self.d, r0=r0, r1=r1,
                 range_bytes=nbytes, out=vp(buf.data_ptr() + start), out_bytes=nbytes + SLACK, flags=p(self.flags))
        a.update(override)
        rc = _lib.lib().kgdet_coco_json_write(i32(a['kind']), a['rows'], i64(a['N']), i32(a['M']), i32(a['W']), a['vals'],
                                              a['rec_src'], a['offset'], a['img'], a['cat'], i32(a['L']), i32(a['d']),
                                              i64(a['r0']), i64(a['r1']), i64(a['range_bytes']), a['out'], i64(a['out_bytes']),
                                              a['flags'], _lib.current_stream())
        host = buf.cpu().numpy()
        assert (host[:start] == CANARY).all() and (host[start + nbytes + SLACK:] == CANARY).all(), 'a canary was overwritten'
        assert (host[start + nbytes:start + nbytes + SLACK] == FILL).all(), 'bytes behind the range were written'
        return rc, host[start:start + nbytes].tobytes()


def _want(c, num_digits=4):
    """per kind (the records with their separators, their offsets, the file's body)"""
    out = []
    for recs in evd._json_records(c.dataset, c.rows, num_digits, num_labels=c.n_labels):
        ext = [(b', ' if r else b'') + rec for r, rec in enumerate(recs)]
        out.append((recs, np.concatenate([[0], np.cumsum([len(e) for e in ext], dtype=np.int64)]).astype(np.int64), b''.join(ext)))
    return out


@pytest.mark.parametrize('name', jc.NAMES)
def test_record_lengths_equal_the_restatement(name):
    c = jc.case(name)
    m = Measured(c)
    assert (m.flags.cpu().numpy() == 0).all() and (m.order_flags == 0).all()
    lens = m.lens.cpu().numpy()
    for kind, (recs, off, _) in enumerate(_want(c)):
        assert m.R == len(recs) > 0
        assert lens[kind, :m.R].tolist() == [len(r) for r in recs], KINDS[kind]
        assert (lens[kind, m.R:] == 0).all()
        assert np.array_equal(m.off[kind, :m.R + 1], off)
    src = m.rec_src.cpu().numpy()
    assert (src[:m.R] >= 0).all() and len(set(src[:m.R].tolist())) == m.R and (src[m.R:] == -1).all()


@pytest.mark.parametrize('num_digits', [1, 2, 3])
def test_fewer_digits(num_digits):
    c = jc.case('edge')
    m = Measured(c, num_digits=num_digits)
    for kind, (recs, off, body) in enumerate(_want(c, num_digits)):
        assert np.array_equal(m.off[kind, :m.R + 1], off)
        assert m.write(kind, 0, m.R, shift=3) == (0, body)
    assert (m.flags.cpu().numpy() == 0).all()


@pytest.mark.parametrize('name', jc.NAMES)
def test_written_bytes_for_the_full_range_and_every_split(name):
    """the full range at destination addresses 0, 1 and 7 mod 16 (the copy-out's head and tail paths differ there); every split
    [0, s) + [s, R) with the second range at its file offset mod 16, as a file-aligned buffer would place it"""
    c = jc.case(name)
    m = Measured(c)
    for kind, (recs, off, body) in enumerate(_want(c)):
        for shift in (0, 1, 7):
            assert m.write(kind, 0, m.R, shift) == (0, body), (KINDS[kind], shift)
        starts = set()
        for s in range(m.R + 1):
            rc0, head = m.write(kind, 0, s, 0)
            rc1, tail = m.write(kind, s, m.R, int(off[s] % 16))
            assert rc0 == rc1 == 0 and head == body[:off[s]] and tail == body[off[s]:], (KINDS[kind], s)
            starts.add(int(off[s] % 16))
        assert 0 in starts and any(s % 2 for s in starts)            # (a first record at a multiple of 16 and at an odd offset)
    assert (m.flags.cpu().numpy() == 0).all()


def test_flag_word_counts_landmark_values_outside_the_domain_once_each():
    c = jc.case('k22')
    assert (Measured(c).flags.cpu().numpy() == 0).all()             # (NaN and 2^40 beyond the counts: not counted)
    for value in jc.OUTSIDE:
        rows = c.rows.copy()
        rows[0, 2, 7 + 40] = value
        m = Measured(c, rows)
        assert m.flags.cpu().numpy().tolist() == [1, 0] and (m.order_flags == 0).all(), value
    rows = c.rows.copy()
    rows[2, 1, 9] = np.nan                                          # (a row with label -1: not written, not counted)
    rows[2, 4, 7:10] = jc.OUTSIDE
    assert Measured(c, rows).flags.cpu().numpy().tolist() == [3, 0]


def test_argument_checks_refuse_before_any_launch(tmp_path):
    c = jc.case('k1')
    m = Measured(c)
    for d in (True, 4.0):                                           # (num_digits is an int: the wrapper's refusal)
        with pytest.raises(ValueError):
            evd.write_device_results_json(c.dataset, DeviceResults(m.rows, c.n_labels + 1), str(tmp_path / 'dev'), num_digits=d)
    assert os.listdir(str(tmp_path)) == []
    null = vp(0)
    want = _want(c)[1][2]
    refused = [m.write(1, 0, m.R, override=kw) for kw in (
        dict(d=0), dict(d=5), dict(W=m.W + 1), dict(W=7), dict(W=7 + 3 * (_lib.COCO_JSON_MAX_K + 1)), dict(M=0),
        dict(M=_lib.COCO_ORDER_MAX_ROWS + 1), dict(L=0), dict(L=_lib.COCO_ORDER_MAX_LABELS + 1), dict(N=-1), dict(kind=2),
        dict(rows=null), dict(vals=null), dict(rec_src=null), dict(offset=null), dict(img=null), dict(cat=null), dict(out=null),
        dict(flags=null), dict(r0=3, r1=2), dict(r0=-1), dict(r1=m.cap + 1), dict(out_bytes=len(want) - 1), dict(range_bytes=-1))]
    assert [rc for rc, _ in refused] == [_lib.KGDET_E_SHAPE] * len(refused)
    assert all(body == bytes([FILL]) * len(body) for _, body in refused)
    assert m.write(1, 2, 2) == (0, b'') and m.write(0, 0, 0, override=dict(rows=null)) == (0, b'')
    assert m.write(1, 0, m.R, override=dict(N=0, rows=null))[0] == 0
    lib, p = _lib.lib(), _lib.ptr
    lens = torch.full((2, m.cap), -7, dtype=torch.int32, device='cuda')
    base = torch.zeros(m.N, dtype=torch.int64, device='cuda')
    info = torch.zeros((m.N, m.M, 3), dtype=torch.int32, device='cuda')

    def measure(**kw):
        a = dict(rows=p(m.rows), N=m.N, M=m.M, W=m.W, vals=p(m.vals), info=p(info), base=p(base), img=p(m.img), cat=p(m.cat),
                 L=m.L, d=4, len_b=p(lens[0]), len_k=p(lens[1]), src=p(m.rec_src), cap=m.cap, flags=p(m.flags))
        a.update(kw)
        return lib.kgdet_coco_json_measure(a['rows'], i64(a['N']), i32(a['M']), i32(a['W']), a['vals'], a['info'], a['base'],
                                           a['img'], a['cat'], i32(a['L']), i32(a['d']), a['len_b'], a['len_k'], a['src'],
                                           i64(a['cap']), a['flags'], _lib.current_stream())

    refused = [measure(**kw) for kw in (
        dict(d=0), dict(d=5), dict(W=m.W + 2), dict(W=7), dict(M=0), dict(M=_lib.COCO_ORDER_MAX_ROWS + 1), dict(L=0),
        dict(L=_lib.COCO_ORDER_MAX_LABELS + 1), dict(N=-1), dict(cap=-1), dict(rows=null), dict(vals=null), dict(info=null),
        dict(base=null), dict(img=null), dict(cat=null), dict(len_b=null), dict(len_k=null), dict(src=null), dict(flags=null))]
    assert refused == [_lib.KGDET_E_SHAPE] * len(refused)
    assert measure(N=0, rows=null) == 0
    torch.cuda.synchronize()
    assert (lens.cpu().numpy() == -7).all() and (m.flags.cpu().numpy() == 0).all()


# ------------------------------------------------------------------------------------------------
# write_device_results_json / results2json_any
# ------------------------------------------------------------------------------------------------
def _same_files(got, want):
    assert set(got) == set(want) == {'bbox', 'proposal', 'keypoints'} and got['proposal'] == got['bbox']
    for kind in KINDS:
        assert filecmp.cmp(got[kind], want[kind], shallow=False), kind


def _json_in(path):
    return sorted(f for f in os.listdir(str(path)) if f.endswith('.json'))


@pytest.mark.parametrize('name', jc.NAMES)
def test_write_device_results_json_equals_results2json(name, tmp_path):
    c = jc.case(name)
    dev = DeviceResults(torch.from_numpy(c.rows).cuda(), c.n_labels + 1)
    want = ev.results2json(c.dataset, dev.to_host(), str(tmp_path / 'host'))
    _same_files(evd.write_device_results_json(c.dataset, dev, str(tmp_path / 'dev')), want)
    assert dev.rows is not None
    longest = max(int(np.diff(off).max()) for _, off, _ in _want(c))
    timings = {}
    _same_files(evd.write_device_results_json(c.dataset, dev, str(tmp_path / 'small'), chunk_bytes=longest, timings=timings), want)
    assert timings['bytes'] == sum(os.path.getsize(want[k]) for k in KINDS)
    before = sorted(os.listdir(str(tmp_path)))
    with pytest.raises(ValueError):
        evd.write_device_results_json(c.dataset, dev, str(tmp_path / 'short'), chunk_bytes=longest - 1)
    assert sorted(os.listdir(str(tmp_path))) == before


def test_an_empty_set_on_the_device(tmp_path):
    c = jc.empty_case()
    files = evd.write_device_results_json(c.dataset, DeviceResults(torch.from_numpy(c.rows).cuda(), c.n_labels + 1),
                                          str(tmp_path / 'dev'))
    for kind in KINDS:
        with open(files[kind], 'rb') as f:
            assert f.read() == b'[]'


def test_what_the_device_route_refuses_goes_down_the_host_route_with_one_warning(tmp_path):
    c = jc.case('k22')
    rows = c.rows.copy()
    rows[4, 6, 7 + 65] = np.inf
    dev = DeviceResults(torch.from_numpy(rows).cuda(), c.n_labels + 1)
    with pytest.raises(ValueError):
        evd.write_device_results_json(c.dataset, dev, str(tmp_path / 'dev'))
    bad_count = c.rows.copy()
    bad_count[0, 0, 6] = jc.M + 1
    for args in ((c.dataset, DeviceResults(torch.from_numpy(bad_count).cuda(), c.n_labels + 1)),
                 (c.dataset, DeviceResults(torch.from_numpy(c.rows).cuda(), c.n_labels + 2)),
                 (jc.Dataset([0, 7, -2, 9, 99], c.dataset.cat_ids), DeviceResults(torch.from_numpy(c.rows).cuda(), c.n_labels + 1))):
        with pytest.raises(ValueError):
            evd.write_device_results_json(args[0], args[1], str(tmp_path / 'dev'))
    for d in (0, 5):
        with pytest.raises(ValueError):
            evd.write_device_results_json(c.dataset, dev, str(tmp_path / 'dev'), num_digits=d)
    assert os.listdir(str(tmp_path)) == []
    want = ev.results2json(c.dataset, dev.to_host(), str(tmp_path / 'host'))
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        got = evd.results2json_any(c.dataset, dev, str(tmp_path / 'any'))
    seen = [w for w in seen if issubclass(w.category, RuntimeWarning)]
    assert len(seen) == 1 and 'not finite' in str(seen[0].message)
    _same_files(got, want)
    assert _json_in(tmp_path) == ['any.bbox.json', 'any.keypoints.json', 'host.bbox.json', 'host.keypoints.json']
    dev.release()
    with pytest.raises(ValueError):
        evd.write_device_results_json(c.dataset, dev, str(tmp_path / 'gone'))


def test_packing_and_writing_in_turn_on_the_same_rows(tmp_path):
    """``kgdet_coco_order_dets`` has one launch site, which serves the packing (the ground truth's tables) and the files
    (identity tables) -- here in turn, in one process, on the same rows: each result against its restatement"""
    c = jc.case('k1')
    data = pack.Dataset(ev.CocoIndex(pack.ground_truth(jc.IMG_IDS, 0)), c.dataset.img_ids, c.dataset.cat_ids)
    pg = pack.packed_gt(pack.Case(dataset=data, K=c.K))
    want_packed = evd.pack_rows_restatement(pg, data, c.rows, 4, num_labels=c.n_labels)
    want_files = evd.json_restatement(data, c.rows, 4, num_labels=c.n_labels)
    assert 0 < len(want_packed['bbox'].score) < int(np.nansum(c.rows[:, 0, 6]))     # (some rows have no ground-truth category)
    dev = DeviceResults(torch.from_numpy(c.rows).cuda(), c.n_labels + 1)
    assert_same_packed(evd.pack_device_results(pg, data, dev), want_packed, 'before the files')
    files = evd.write_device_results_json(data, dev, str(tmp_path / 'dev'))
    for kind, want in zip(KINDS, want_files):
        with open(files[kind], 'rb') as f:
            assert f.read() == want, kind
    assert_same_packed(evd.pack_device_results(pg, data, dev), want_packed, 'after the files')


# ------------------------------------------------------------------------------------------------
# the route: detector -> DeviceResults -> the two files, on the demo set
# ------------------------------------------------------------------------------------------------
def _to_dev(t):
    return t.cuda(non_blocking=True)


def test_demo_set_files_equal_the_plain_runs(tmp_path):
    """detections as tests/test_gpu_eval_pack.py's ``demo`` fixture obtains them; the second call hands the device route a
    dataset stub without annotations"""
    cfg, model = demo_cases.demo_detector()
    model = model.cuda()
    data = demo_cases.demo_dataset(test_mode=True)
    plain = single_gpu_test(model, data, rescale=True, to_device=_to_dev, imgs_per_gpu=4)
    dev = single_gpu_test(model, data, rescale=True, to_device=_to_dev, imgs_per_gpu=4, device_results=True)
    assert isinstance(dev, DeviceResults) and dev.rows.is_cuda
    want = ev.results2json(data, plain, str(tmp_path / 'plain'))
    assert os.path.getsize(want['keypoints']) > 1 << 20
    _same_files(evd.write_device_results_json(data, dev, str(tmp_path / 'dev')), want)
    stub = jc.Dataset(data.img_ids, data.cat_ids)
    _same_files(evd.write_device_results_json(stub, dev, str(tmp_path / 'stub'), chunk_bytes=1 << 18), want)
    _same_files(evd.results2json_any(stub, dev, str(tmp_path / 'any')), want)


def _tool(name):
    spec = importlib.util.spec_from_file_location('kgdet_tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_test_tool_with_device_results_leaves_the_same_files(tmp_path):
    """(at the config's own scale, where the detector repeats itself bit for bit -- tests/test_gpu_loader.py; the first run
    only visits the shapes)"""
    ann, prefix = lc.write_image_dir(str(tmp_path / 'set'), n=4)
    config = lc.write_config_file(str(tmp_path / 'demo.py'), lc.demo_config(ann, prefix, str(tmp_path / 'work'),
                                                                            img_scale=demo_cases.IMG_SCALE))
    ckpt = str(tmp_path / 'demo.pth')
    save_checkpoint(demo_cases.demo_detector()[1], ckpt)
    tool = _tool('test')
    tool.main([config, ckpt, '--json_out', str(tmp_path / 'warm')])
    tool.main([config, ckpt, '--json_out', str(tmp_path / 'host')])
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)              # (the host route's warning would be a failure)
        tool.main([config, ckpt, '--device-results', '--json_out', str(tmp_path / 'dev.json')])
    for kind in KINDS:
        assert os.path.getsize(str(tmp_path / ('host.%s.json' % kind))) > 2
        assert filecmp.cmp(str(tmp_path / ('dev.%s.json' % kind)), str(tmp_path / ('host.%s.json' % kind)), shallow=False), kind
