"""``kgdet_coco_order_dets`` / ``kgdet_coco_scatter_dets`` (csrc/coco_pack_dets.hip) through the C ABI, and the route they
serve: ``single_gpu_test(..., device_results=True)`` -> ``evaluate_results``.

The bar is EQUALITY of bits with ``pack_rows_restatement`` (held to the host packing and to Python's ``round`` on the CPU by
tests/test_eval_pack_refs.py): the rounding is exact by construction (one FMA residual, one correctly rounded division,
compiled without contraction), everything else is integers and copies.  Outputs are pre-filled with NaN / -1 between
canaries: every element must be written and nothing beside them."""
import ctypes

import numpy as np
import pytest
import torch

from kgdet_amd import _lib
from kgdet_amd import evaluation_device as evd
from kgdet_amd.runner import DeviceResults, single_gpu_test
from tests import eval_pack_cases as pack
from tests.golden import demo_cases
from tests.test_eval_pack_refs import assert_same_packed, same_bits

pytestmark = pytest.mark.gpu
PAD = 64                                  # (elements; even, so a float32 block keeps the 8-byte alignment of its buffer)
i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
CANARY = {torch.float64: -12345.5, torch.float32: -12345.5, torch.int64: -777, torch.int32: -777}
FILL = {torch.float64: float('nan'), torch.float32: float('nan'), torch.int64: -1, torch.int32: -1}


class Guarded(object):
    """an allocator for ``_pack_rows_on_device``: every block sits between canaries in a buffer of its own, pre-filled"""

    def __init__(self):
        self.blocks = []

    def __call__(self, shape, dtype):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), CANARY[dtype], dtype=dtype, device='cuda')
        buf[PAD:PAD + n] = FILL[dtype]
        self.blocks.append((buf, n))
        return buf[PAD:PAD + n].view(shape)

    def check(self):
        for buf, n in self.blocks:
            host = buf.cpu().numpy()
            assert (host[:PAD] == CANARY[buf.dtype]).all() and (host[PAD + n:] == CANARY[buf.dtype]).all(), 'a canary was overwritten'


def _tables(c, pg):
    return evd._pack_tables(pg, c.dataset, c.rows.shape[0], c.n_labels)


def _device_packed(c, pg, rows=None):
    """the kernels on a case through the C ABI, outputs guarded -> {'bbox': Packed, 'keypoints': Packed} on the host"""
    slot, col = _tables(c, pg)
    alloc = Guarded()
    C = len(pg.cat_ids)
    outs, start = evd._pack_rows_on_device(torch.from_numpy(c.rows if rows is None else rows).cuda(), slot, col, C,
                                           len(pg.img_ids) * C, 4, alloc=alloc)
    torch.cuda.synchronize()
    alloc.check()
    host = [{f: (t.cpu().numpy() if t is not None else None) for f, t in o.items()} for o in outs]
    for o in host:
        for f in ('cell', 'img_idx', 'cat_idx', 'id'):
            assert (o[f] >= 0).all(), '%s: an element was not written' % f
        for f in ('score', 'bbox', 'area', 'kxy32'):
            assert o[f] is None or not np.isnan(o[f]).any(), '%s: an element was not written' % f
    kxy32 = host[1].pop('kxy32')
    return evd._packed_pair(host, start.cpu().numpy(), kxy32, 4)


@pytest.mark.parametrize('name', pack.NAMES)
def test_kernels_equal_the_restatement(name):
    c = pack.case(name)
    pg = pack.packed_gt(c)
    want = evd.pack_rows_restatement(pg, c.dataset, c.rows, 4)
    assert_same_packed(_device_packed(c, pg), want, name)


def test_pack_device_results_equals_the_host_packing_and_keeps_the_landmarks_on_the_device():
    c = pack.case('mixed')
    pg = pack.packed_gt(c)
    got = evd.pack_device_results(pg, c.dataset, DeviceResults(torch.from_numpy(c.rows).cuda(), c.n_labels + 1))
    assert torch.is_tensor(got['keypoints'].kxy32) and got['keypoints'].kxy32.is_cuda
    assert isinstance(got['bbox'].score, np.ndarray) and isinstance(got['keypoints'].cell, np.ndarray)
    assert_same_packed(got, evd.pack_test_results(pg, c.dataset, c.results, 4, lazy_landmarks=True), 'mixed')


def _order_flags(rows, c, pg):
    """kgdet_coco_order_dets alone -> its flag words"""
    N, M, W = rows.shape
    slot, col = evd._pack_tables(pg, c.dataset, N, c.n_labels)
    C = len(pg.cat_ids)
    dev = dict(rows=torch.from_numpy(rows).cuda(), slot=torch.from_numpy(slot).cuda(), col=torch.from_numpy(col).cuda(),
               vals=torch.empty((N, M, 6), dtype=torch.float64, device='cuda'),
               info=torch.empty((N, M, 3), dtype=torch.int32, device='cuda'),
               img_rows=torch.empty(N, dtype=torch.int32, device='cuda'),
               cnt=torch.zeros((2, len(pg.img_ids) * C), dtype=torch.int32, device='cuda'),
               flags=torch.zeros(2, dtype=torch.int32, device='cuda'))
    p = _lib.ptr
    rc = _lib.lib().kgdet_coco_order_dets(p(dev['rows']), i64(N), i32(M), i32(W), p(dev['slot']), p(dev['col']), i32(len(col)),
                                          i32(C), i64(len(pg.img_ids) * C), i32(4), i32(100), i32(20), p(dev['vals']),
                                          p(dev['info']), p(dev['img_rows']), p(dev['cnt'][0]), p(dev['cnt'][1]),
                                          p(dev['flags']), _lib.current_stream())
    assert rc == 0, _lib.lib().kgdet_last_error()
    return dev['flags'].cpu().numpy()


@pytest.mark.parametrize('column,value', [(4, np.inf), (0, 2e8), (3, np.nan)])
def test_flag_word_for_values_outside_the_rounding_domain(column, value):
    c = pack.case('ties')
    pg = pack.packed_gt(c)
    assert (_order_flags(c.rows, c, pg) == 0).all()
    rows = c.rows.copy()
    rows[1, 2, column] = value
    flags = _order_flags(rows, c, pg)
    assert flags[0] >= 1 and flags[1] == 0
    with pytest.raises(ValueError):
        evd.pack_device_results(pg, c.dataset, DeviceResults(torch.from_numpy(rows).cuda(), c.n_labels + 1))


def test_flag_word_for_a_count_beyond_the_rows_and_an_unknown_image():
    c = pack.case('ties')
    pg = pack.packed_gt(c)
    rows = c.rows.copy()
    rows[0, 0, 6] = c.M + 1
    assert _order_flags(rows, c, pg)[1] == 1
    other = pack.Case(dataset=pack.Dataset(c.dataset.coco, [12345] + c.dataset.img_ids[1:], c.dataset.cat_ids),
                      n_labels=c.n_labels)
    assert _order_flags(c.rows, other, pg)[1] == 1
    with pytest.raises(ValueError):
        evd.pack_device_results(pg, other.dataset, DeviceResults(torch.from_numpy(c.rows).cuda(), c.n_labels + 1))


def test_evaluate_results_takes_the_host_route_for_what_the_kernels_refuse():
    c = pack.case('mixed')
    pg = pack.packed_gt(c)
    rows = c.rows.copy()
    rows[0, 16, 2] = 3e8                           # (x2 of a false positive: its width leaves the rounding's domain)
    dev = DeviceResults(torch.from_numpy(rows).cuda(), c.n_labels + 1)
    want = evd.evaluate_results(c.dataset, dev.to_host(), device='cuda', packed_gt=pg)
    got = evd.evaluate_results(c.dataset, dev, device='cuda', packed_gt=pg)
    assert dev.rows is None
    for t in ('bbox', 'keypoints'):
        assert np.array_equal(got[t], want[t]), t


def test_argument_checks_refuse_before_any_launch():
    c = pack.case('ties')
    pg = pack.packed_gt(c)
    slot, col = _tables(c, pg)
    N, M, W = c.rows.shape
    C, n_cells = len(pg.cat_ids), len(pg.img_ids) * len(pg.cat_ids)
    L = _lib.lib()
    alloc = Guarded()
    t = dict(rows=torch.from_numpy(c.rows).cuda(), slot=torch.from_numpy(slot).cuda(), col=torch.from_numpy(col).cuda(),
             vals=alloc((N, M, 6), torch.float64), info=alloc((N, M, 3), torch.int32), img_rows=alloc((N,), torch.int32),
             cnt_b=alloc((n_cells,), torch.int32), cnt_k=alloc((n_cells,), torch.int32), flags=alloc((2,), torch.int32),
             img_base=torch.zeros(N, dtype=torch.int64, device='cuda'),
             start=torch.zeros(n_cells + 1, dtype=torch.int64, device='cuda'))
    out = {f: alloc((8,) if f != 'bbox' else (8, 4), torch.int64 if f in ('cell', 'img_idx', 'cat_idx', 'id') else torch.float64)
           for f in ('cell', 'img_idx', 'cat_idx', 'id', 'score', 'bbox', 'area')}
    out['kxy32'] = alloc((8, W - 7), torch.float32)
    p = _lib.ptr

    def order(**kw):
        a = dict(rows=p(t['rows']), N=N, M=M, W=W, slot=p(t['slot']), col=p(t['col']), L=len(col), C=C, n_cells=n_cells, d=4,
                 cut_b=100, cut_k=20, vals=p(t['vals']), info=p(t['info']), img_rows=p(t['img_rows']), cnt_b=p(t['cnt_b']),
                 cnt_k=p(t['cnt_k']), flags=p(t['flags']))
        a.update(kw)
        return L.kgdet_coco_order_dets(a['rows'], i64(a['N']), i32(a['M']), i32(a['W']), a['slot'], a['col'], i32(a['L']),
                                       i32(a['C']), i64(a['n_cells']), i32(a['d']), i32(a['cut_b']), i32(a['cut_k']), a['vals'],
                                       a['info'], a['img_rows'], a['cnt_b'], a['cnt_k'], a['flags'], _lib.current_stream())

    def scatter(n=8, **kw):
        s = [_lib.CocoPackedDets(n=n, **{f: out[f].data_ptr() for f in out}) for _ in range(2)]
        a = dict(rows=p(t['rows']), N=N, M=M, W=W, slot=p(t['slot']), C=C, n_cells=n_cells, vals=p(t['vals']), info=p(t['info']),
                 img_base=p(t['img_base']), start_b=p(t['start']), start_k=p(t['start']), cut_b=100, cut_k=20,
                 out_b=ctypes.byref(s[0]), out_k=ctypes.byref(s[1]), flags=p(t['flags']))
        a.update(kw)
        return L.kgdet_coco_scatter_dets(a['rows'], i64(a['N']), i32(a['M']), i32(a['W']), a['slot'], i32(a['C']), i64(a['n_cells']),
                                         a['vals'], a['info'], a['img_base'], a['start_b'], a['start_k'], i32(a['cut_b']),
                                         i32(a['cut_k']), a['out_b'], a['out_k'], a['flags'], _lib.current_stream())

    null = vp(0)
    refused = [order(d=0), order(d=10), order(M=_lib.COCO_ORDER_MAX_ROWS + 1), order(M=0), order(L=_lib.COCO_ORDER_MAX_LABELS + 1),
               order(L=0), order(W=W + 1), order(W=7), order(N=-1), order(n_cells=-1), order(C=0), order(cut_b=-1),
               order(rows=null), order(slot=null), order(col=null), order(vals=null), order(info=null), order(img_rows=null),
               order(cnt_b=null), order(flags=null),
               scatter(M=_lib.COCO_ORDER_MAX_ROWS + 1), scatter(W=W + 2), scatter(N=-1), scatter(C=0), scatter(cut_k=-1),
               scatter(n=-1), scatter(rows=null), scatter(vals=null), scatter(info=null), scatter(img_base=null),
               scatter(start_b=null), scatter(flags=null), scatter(out_b=ctypes.POINTER(_lib.CocoPackedDets)())]
    assert refused == [_lib.KGDET_E_SHAPE] * len(refused), refused
    assert order(N=0, rows=null) == 0 and scatter(N=0, rows=null) == 0            # (N == 0: a no-op)
    for d in (True, 4.0):                                                         # (num_digits is an int: the wrapper's refusal)
        with pytest.raises(ValueError):
            evd.pack_device_results(pg, c.dataset, DeviceResults(t['rows'], c.n_labels + 1), num_digits=d)
    torch.cuda.synchronize()
    alloc.check()
    for buf, n in alloc.blocks:                                                   # nothing was launched: the fill is intact
        body = buf[PAD:PAD + n].cpu().numpy()
        assert np.isnan(body).all() if body.dtype.kind == 'f' else (body == -1).all()


# ------------------------------------------------------------------------------------------------
# the route: detector -> DeviceResults -> evaluate_results, on the demo set
# ------------------------------------------------------------------------------------------------
class _Slice(object):
    """samples ``indices`` of a dataset, everything else the dataset's own"""

    def __init__(self, data, indices):
        self._data, self._indices = data, list(indices)
        self.img_ids = [data.img_ids[i] for i in indices]

    def __len__(self):
        return len(self._indices)

    def __getitem__(self, i):
        return self._data[self._indices[i]]

    def prepare_test_raw(self, i):
        return self._data.prepare_test_raw(self._indices[i])

    def __getattr__(self, name):
        return getattr(self._data, name)


def _to_dev(t):
    return t.cuda(non_blocking=True)


def _assert_same_results(got, want):
    assert len(got) == len(want)
    n = 0
    for g, w in zip(got, want):
        assert type(g) is tuple and len(g) == len(w)
        for part_g, part_w in zip(g, w):
            for x, y in (zip(part_g, part_w) if isinstance(part_w, list) else [(part_g, part_w)]):
                assert same_bits(x, y)
        n += len(w[1]) if len(w) == 3 else 0
    return n


@pytest.fixture(scope='module')
def demo():
    """the demo detector and set, the plain list of one run and the rows of a device-results run (a CPU copy, left unchanged)"""
    cfg, model = demo_cases.demo_detector()
    model = model.cuda()
    data = demo_cases.demo_dataset(test_mode=True)
    want = single_gpu_test(model, data, rescale=True, to_device=_to_dev, imgs_per_gpu=4)
    dev = single_gpu_test(model, data, rescale=True, to_device=_to_dev, imgs_per_gpu=4, device_results=True)
    assert isinstance(dev, DeviceResults) and dev.rows.is_cuda
    assert dev.rows.shape == (32, cfg.test_cfg.max_per_img, 7 + 3 * 294) and dev.rows.dtype == torch.float32
    return dict(model=model, data=data, want=want, rows=dev.rows.cpu(), num_classes=dev.num_classes, dev=dev)


def test_device_results_to_host_is_the_plain_list(demo):
    assert _assert_same_results(demo['dev'].to_host(), demo['want']) == 401


@pytest.mark.parametrize('device_accumulate', [True, False])
def test_evaluate_results_on_device_results_equals_the_list_route(demo, device_accumulate):
    data = demo['data']
    want = evd.evaluate_results(data, demo['want'], device='cuda', lazy_landmarks=True, device_accumulate=device_accumulate)
    dev = DeviceResults(demo['rows'].cuda(), demo['num_classes'])
    got = evd.evaluate_results(data, dev, device='cuda', device_accumulate=device_accumulate)
    assert dev.rows is None
    for t in ('bbox', 'keypoints'):
        assert np.array_equal(got[t], want[t]), (t, got[t], want[t])


def test_packing_the_demo_rows_equals_packing_the_plain_list(demo):
    """(the demo detector's weights are seeded, not trained: its stats say little, so the packed arrays themselves are compared)"""
    data = demo['data']
    pg = evd.pack_ground_truth(data.coco)
    got = evd.pack_device_results(pg, data, DeviceResults(demo['rows'].cuda(), demo['num_classes']))
    assert len(got['bbox'].score) == 401 and got['keypoints'].kxy32.is_cuda
    assert_same_packed(got, evd.pack_test_results(pg, data, demo['want'], 4, lazy_landmarks=True), 'demo')


@pytest.mark.parametrize('device_preprocess', [False, True])
def test_one_image_per_forward_and_device_preprocess_compose(demo, device_preprocess):
    data = _Slice(demo['data'], [0, 5, 9])
    kw = dict(rescale=True, to_device=_to_dev, device_preprocess=device_preprocess)
    want = single_gpu_test(demo['model'], data, **kw)
    got = single_gpu_test(demo['model'], data, device_results=True, **kw)
    assert got.rows.shape[0] == 3
    _assert_same_results(got.to_host(), want)


def test_a_tta_sample_and_a_sample_off_the_packed_path(demo, monkeypatch):
    model = demo['model']
    tta = _Slice(demo_cases.demo_dataset(test_mode=True, flip_ratio=0.5), [3])
    want = single_gpu_test(model, tta, rescale=True, to_device=_to_dev)
    got = single_gpu_test(model, tta, rescale=True, to_device=_to_dev, device_results=True)
    assert _assert_same_results(got.to_host(), want) > 0
    one = _Slice(demo['data'], [3])
    monkeypatch.setattr(model.bbox_head, '_packed_ok', lambda *a, **k: False)      # (both runs leave the fused NMS for the per-image results)
    want = single_gpu_test(model, one, rescale=True, to_device=_to_dev)
    got = single_gpu_test(model, one, rescale=True, to_device=_to_dev, device_results=True)
    assert _assert_same_results(got.to_host(), want) > 0


def test_more_detections_than_rows_or_no_row_limit_is_refused(demo, monkeypatch):
    model = demo['model']
    det = torch.zeros((5, 5), device='cuda')
    with pytest.raises(NotImplementedError):
        model.pack_detections(det, torch.zeros(5, device='cuda'), torch.zeros((5, 882), device='cuda'), 4)
    cfg = type(model.test_cfg)(dict(model.test_cfg))
    cfg['max_per_img'] = -1
    monkeypatch.setattr(model, 'test_cfg', cfg)
    with pytest.raises(NotImplementedError):
        single_gpu_test(model, _Slice(demo['data'], [0]), rescale=True, to_device=_to_dev, device_results=True)
