"""The table route of the fused head-loss kernels -- kgdet_head_loss_forward_table / _backward_table (csrc/head_loss.hip): the
per-image ground-truth counts and valid extents come from a DEVICE table [B][4] = (num_gt, valid_h, valid_w, 0), the ground
truth lies in buffers of ``gt_capacity`` rows -- against the by-value route (kgdet_head_loss_forward / _backward) on the same
inputs, bit for bit: the nine losses, num_total, every selection row g < num_gt and the nine gradient maps.

tests/test_gpu_head_loss_kernels.py holds the by-value route to the float64 reference of tests/head_loss_refs.py; equality
carries that over.  Rows beyond an image's count are NaN boxes, NaN keypoints and label 2^40 (or whatever an earlier call left
there): a kernel that read one would show it.  Outputs and workspace sit inside canaries and are pre-filled with NaN.  No test
feeds the kernels a table outside its range.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import head_loss_refs as R

pytestmark = pytest.mark.gpu

CANARY = 12345.678
BAD_LABEL = 2 ** 40


def _L():
    from kgdet_amd import _lib
    return _lib, _lib.lib()


class Guarded(object):
    """``n`` floats of NaN at 64 floats into a buffer of CANARY"""

    def __init__(self, n, lead=64, tail=64):
        self.n, self.lead = n, lead
        self.buf = torch.full((lead + n + tail,), CANARY, dtype=torch.float32, device='cuda')
        self.view().fill_(float('nan'))

    def view(self):
        return self.buf[self.lead:self.lead + self.n]

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lead

    def intact(self):
        return bool((self.buf[:self.lead] == CANARY).all()) and bool((self.buf[self.lead + self.n:] == CANARY).all())

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.view()).all())


class Route(object):
    """the device side of one route for cases of one shape: ``cap=None`` the by-value route (ground truth of exactly num_gt rows,
    counts and extents in the descriptor), else the table route (buffers of ``cap`` rows, a device table).  ``write(case)``
    puts a case's contents into the SAME buffers; rows beyond the count keep what they held (NaN / 2^40 at first)."""

    def __init__(self, case, cap=None, labels=True):
        from kgdet_amd import head_loss as HL
        lib, L = _L()
        self.cap, self.B, self.shape = cap, case.B, (case.H, case.W, case.C, case.K)
        B, (H, W, C, K) = case.B, self.shape
        t = HL.HeadTargets()
        t.B, t.H, t.W, t.num_classes, t.num_keypoints, t.stride = B, H, W, C, K, case.stride
        self.t, self.c = t, HL.HeadLossCfg()
        rows = cap if cap is not None else R.MAX_GT
        self.bb = [torch.full((rows, 4), float('nan'), dtype=torch.float32, device='cuda') for _ in range(B)]
        self.kp = [torch.full((rows, K, 3), float('nan'), dtype=torch.float32, device='cuda') for _ in range(B)]
        self.lab = [torch.full((rows, ), BAD_LABEL, dtype=torch.int64, device='cuda') for _ in range(B)] if labels else None
        for b in range(B):
            t.gt_bboxes[b], t.gt_keypoints[b] = self.bb[b].data_ptr(), self.kp[b].data_ptr()
            t.gt_labels[b] = self.lab[b].data_ptr() if labels else None
        self.table = torch.zeros((B, 4), dtype=torch.int32, device='cuda') if cap is not None else None
        self.maps = [torch.zeros((B, ch, H, W), dtype=torch.float32, device='cuda') for ch in (C,) * 3 + (4,) * 3 + (2 * K,) * 3]
        self.hm = HL._maps(self.maps)
        self.up = torch.zeros(9, dtype=torch.float32, device='cuda')
        self.ws_bytes = L.kgdet_head_loss_workspace_bytes(ctypes.byref(t))
        self.ws = Guarded((self.ws_bytes + 3) // 4)
        self.out = Guarded(10)
        self.grads = [Guarded(m.numel()) for m in self.maps]
        hg = HL.HeadMaps()
        for s in range(3):
            hg.cls[s], hg.bbox[s], hg.kpt[s] = self.grads[s].ptr(), self.grads[3 + s].ptr(), self.grads[6 + s].ptr()
        self.hg = hg
        self.write(case)

    def write(self, case):
        """a case's contents, by copies on the current stream (pointers and shapes stay)"""
        assert (case.H, case.W, case.C, case.K) == self.shape and case.B == self.B
        dev = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
        t, c = self.t, self.c
        self.counts = [len(bx) for bx in case.boxes]
        for b in range(self.B):
            n = self.counts[b]
            assert self.cap is None or n <= self.cap
            self.bb[b][:n].copy_(dev(case.boxes[b]))
            self.kp[b][:n].copy_(dev(case.kps[b]))
            if self.lab is not None:
                self.lab[b][:n].copy_(dev(case.labels[b], np.int64))
            if self.cap is None:
                t.num_gt[b] = n
                t.valid_h[b], t.valid_w[b] = case.valid[b]
            else:                        # (the by-value fields are ignored on the table route: poison them)
                t.num_gt[b], t.valid_h[b], t.valid_w[b] = -7, -3, 100000
        if self.cap is not None:
            rows = [[self.counts[b], case.valid[b][0], case.valid[b][1], 0] for b in range(self.B)]
            self.table.copy_(dev(rows, np.int32))
        c.pos_num, c.pos_weight, c.normalize_term = case.pos_num, case.pos_weight, case.normalize_term
        for s in range(3):
            c.gamma[s], c.alpha[s] = case.gamma[s], case.alpha[s]
        for s in range(6):
            c.beta[s] = case.beta[s]
        for s in range(9):
            c.loss_weight[s] = case.loss_weight[s]
        for m, src in zip(self.maps, [a for k in ('cls', 'bbox', 'kpt') for a in case.maps[k]]):
            m.copy_(dev(src))
        self.up.copy_(dev(np.asarray(case.upstream, np.float32)))

    def forward(self, table='own', cap=None):
        lib, L = _L()
        tail = (ctypes.c_void_p(self.out.ptr()), ctypes.c_void_p(self.out.ptr() + 36), ctypes.c_void_p(self.ws.ptr()),
                ctypes.c_size_t(self.ws_bytes), lib.current_stream())
        if self.cap is None:
            return L.kgdet_head_loss_forward(ctypes.byref(self.t), ctypes.byref(self.c), ctypes.byref(self.hm), *tail)
        tp = self.table.data_ptr() if table == 'own' else table
        return L.kgdet_head_loss_forward_table(ctypes.byref(self.t), ctypes.byref(self.c), ctypes.byref(self.hm),
                                               ctypes.c_void_p(tp), ctypes.c_int32(self.cap if cap is None else cap), *tail)

    def backward(self, table='own', cap=None):
        lib, L = _L()
        tail = (ctypes.c_void_p(self.up.data_ptr()), ctypes.c_void_p(self.out.ptr() + 36), ctypes.byref(self.hg),
                ctypes.c_void_p(self.ws.ptr()), ctypes.c_size_t(self.ws_bytes), lib.current_stream())
        if self.cap is None:
            return L.kgdet_head_loss_backward(ctypes.byref(self.t), ctypes.byref(self.c), ctypes.byref(self.hm), *tail)
        tp = self.table.data_ptr() if table == 'own' else table
        return L.kgdet_head_loss_backward_table(ctypes.byref(self.t), ctypes.byref(self.c), ctypes.byref(self.hm),
                                                ctypes.c_void_p(tp), ctypes.c_int32(self.cap if cap is None else cap), *tail)

    def run(self):
        lib, _ = _L()
        lib.check(self.forward(), 'head_loss forward')
        lib.check(self.backward(), 'head_loss backward')

    def nothing_written(self):
        torch.cuda.synchronize()
        return self.out.untouched() and self.ws.untouched() and all(g.untouched() for g in self.grads)

    def results(self):
        """(losses + num_total [10], [selection rows g < num_gt per image], [nine gradient maps]) as int32 bit patterns"""
        torch.cuda.synchronize()
        H, W = self.shape[:2]
        N = H * W
        d = self.ws.view()[:self.B * R.MAX_GT * N].cpu().numpy().reshape(self.B, R.MAX_GT, N)
        return (self.out.view().cpu().numpy().view(np.int32), [d[b, :self.counts[b]].view(np.int32) for b in range(self.B)],
                [g.view().cpu().numpy().view(np.int32) for g in self.grads])

    def intact(self):
        return self.out.intact() and self.ws.intact() and all(g.intact() for g in self.grads)


def _assert_equal(table_route, value_route, tag):
    a, b = table_route.results(), value_route.results()
    assert table_route.intact() and value_route.intact(), '%s: a canary was overwritten' % tag
    assert np.isfinite(a[0].view(np.float32)).all(), '%s: a loss is not finite' % tag
    assert (a[0] == b[0]).all(), '%s: losses / num_total differ: %s vs %s' % (tag, a[0].view(np.float32), b[0].view(np.float32))
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert x.shape == y.shape and (x == y).all(), '%s: selection rows of image %d differ' % (tag, i)
    for k, (x, y) in enumerate(zip(a[2], b[2])):
        assert np.isfinite(x.view(np.float32)).all(), '%s: gradient map %d holds a NaN or an infinity' % (tag, k)
        assert (x == y).all(), '%s: gradient map %d differs' % (tag, k)


A1_CASES = ['n35_c1k1', 'n35_b16', 'kgdet_config', 'mixed_64_1_7', 'outside', 'one_row_valid', 'pos_num_all_valid',
            'exact_ties', 'identical_64', 'strip_1xW']


@pytest.mark.parametrize('name', A1_CASES)
def test_table_route_equals_the_by_value_route_bit_for_bit(name):
    case = R.make_case(name)
    most = max(len(b) for b in case.boxes)
    cap = 64 if most == 64 else (most + 7) // 8 * 8
    labels = case.labels is not None
    by_table, by_value = Route(case, cap=cap, labels=labels), Route(case, labels=labels)
    by_table.run()
    by_value.run()
    _assert_equal(by_table, by_value, name)
    # the rows beyond the counts were not written either
    for b in range(case.B):
        assert bool(torch.isnan(by_table.bb[b][by_table.counts[b]:]).all())


def _random_case(B, H, W, C, K, counts, valid, seed, pos_num=9, cfg=R.VARIED_CFG):
    """a case of head_loss_refs' form with given counts and extents (random boxes inside the valid extent, every keypoint
    visibility in {0, 1, 2}, normal maps): both routes get the same arrays, no reference is evaluated"""
    rng = np.random.default_rng(seed)
    s = 32.0
    f32 = np.float32
    boxes, labels, kps = [], [], []
    for b in range(B):
        G = counts[b]
        ew, eh = R.extent(valid[b][1], W) * s, R.extent(valid[b][0], H) * s
        cx, cy = rng.uniform(0, ew, G), rng.uniform(0, eh, G)
        w, h = rng.uniform(1.5 * s, 3 * s, G), rng.uniform(1.5 * s, 3 * s, G)
        boxes.append(np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(f32))
        labels.append(rng.integers(1, C + 1, G).astype(np.int64))
        xy = np.stack([rng.uniform(0, W * s, (G, K)), rng.uniform(0, H * s, (G, K))], 2)
        v = rng.integers(0, 3, (G, K)).astype(np.float64)
        kps.append(np.concatenate([xy, v[:, :, None]], 2).astype(f32))
    mk = lambda ch, sc: (rng.standard_normal((B, ch, H, W), dtype=f32) * f32(sc)).astype(f32)
    maps = dict(cls=[mk(C, 2.0) for _ in range(3)], bbox=[mk(4, 4.0) for _ in range(3)], kpt=[mk(2 * K, 4.0) for _ in range(3)])
    return R.Case(name='random', regime='free', B=B, H=H, W=W, C=C, K=K, stride=s, boxes=boxes, valid=valid, labels=labels,
                  kps=kps, pos_num=pos_num, normalize_term=4 * s, maps=maps, **cfg)


SEQUENCE = [((8, 1, 2), [(0, 0), (4, 11), (9, 5)]), ((1, 8, 3), [(9, 11), (0, 0), (3, 4)]), ((2, 2, 1), [(5, 5), (9, 3), (0, 0)])]


def test_one_set_of_buffers_serves_calls_with_other_counts():
    """three calls through the same buffers and the same workspace; the second shrinks image 0 from 8 rows to 1 -- the rows 1..7
    of its buffers and of its selections still hold the first call's values, and must not be read"""
    B, H, W, C, K = 3, 9, 11, 3, 5
    cases = [_random_case(B, H, W, C, K, counts, valid, seed=20 + i) for i, (counts, valid) in enumerate(SEQUENCE)]
    by_table = Route(cases[0], cap=8)
    for i, case in enumerate(cases):
        if i:
            by_table.write(case)
        by_value = Route(case)
        by_table.run()
        by_value.run()
        _assert_equal(by_table, by_value, 'call %d' % i)
    # the stale rows are still there: they were there to be read
    assert bool(torch.isfinite(by_table.bb[0][2:8]).all())


def test_a_captured_graph_replays_on_other_counts_extents_and_maps():
    """forward + backward of the table route captured ONCE; table, ground truth and maps rewritten between replays; every replay
    equals the by-value eager call on the same contents bit for bit"""
    B, H, W, C, K = 3, 5, 7, 2, 3
    seq = [((2, 2, 2), [(0, 0), (0, 0), (0, 0)]), ((8, 1, 2), [(0, 0), (3, 7), (5, 4)]), ((1, 8, 3), [(4, 4), (0, 0), (2, 7)]),
           ((2, 2, 1), [(5, 2), (3, 3), (0, 0)])]
    cases = [_random_case(B, H, W, C, K, counts, valid, seed=40 + i) for i, (counts, valid) in enumerate(seq)]
    by_table = Route(cases[0], cap=8)
    by_table.run()                               # (code objects loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        by_table.run()
    for i, case in enumerate(cases[1:], 1):
        by_table.write(case)
        for g in [by_table.out, by_table.ws] + by_table.grads:
            g.view().fill_(float('nan'))
        graph.replay()
        by_value = Route(case)
        by_value.run()
        _assert_equal(by_table, by_value, 'replay %d' % i)


@pytest.mark.parametrize('what', ['null_table', 'capacity_0', 'capacity_65'])
def test_a_bad_table_argument_is_refused_before_anything_is_written(what):
    from kgdet_amd import _lib
    case = _random_case(2, 5, 7, 2, 3, (2, 1), [(0, 0), (0, 0)], seed=60)
    route = Route(case, cap=8)
    kw = dict(null_table=dict(table=0), capacity_0=dict(cap=0), capacity_65=dict(cap=65))[what]
    assert route.forward(**kw) == _lib.KGDET_E_SHAPE
    assert route.backward(**kw) == _lib.KGDET_E_SHAPE
    assert route.nothing_written()
