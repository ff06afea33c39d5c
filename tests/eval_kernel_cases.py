"""Cases and scalar references for the two entry points of csrc/coco_eval.hip, ``kgdet_coco_similarity`` and ``kgdet_coco_match``,
shared by tests/test_eval_kernel_refs.py (CPU) and tests/test_gpu_eval_kernels.py (the kernels through the C ABI).

A case is a chunk in the layout of ``DeviceCocoEvaluator._chunks`` (cells [C, 4] = first detection, detections, first ground
truth, ground truths; ``sim_off`` [C]; the packed arrays).  The references are NOT ``evaluation_device.similarity_restatement`` /
``match_restatement``, which were written next to the kernels: similarities are ``evaluation.box_iou_xywh`` / ``evaluation.oks``
applied cell by cell, matching is a scalar loop per (area range, threshold) written from ``CocoEvaluator._match`` -- stable sort
of the ground truths by ignore flag, the ``break`` at the first ignored one once a regular match exists, ``sim < best ->
continue``.  The CPU test holds the restatements to them.

What the kernels skip is part of the contract and of the references: a cell whose ranges leave the arrays is not touched at all;
a cell whose ``[sim_off, sim_off + D G)`` leaves ``[0, sim_size]`` gets no similarities, and the matcher then leaves its
detections unmatched (ignored by area alone) while still writing the ground-truth flags.  Outputs start at a fill value, so
"not touched" is visible.

Matching similarities are written by hand on a grid of 1/64, or are exactly a threshold / one float below it, so no decision
depends on a rounding.  Paths: the matcher runs one lane per (a, t), A T = 1 ... 64 (one lane, 30, 40, and a full wave three
ways); the OKS kernel strides K over the 64 lanes of a wave: K = 1 and 63 leave idle lanes, 64 fills the wave, 65 gives lane 0
a second landmark, 294 is the dataset's; 70 x 33 pairs take a workgroup of 256 (IoU) or 4 waves (OKS) through several trips.
"""
import types

import numpy as np

from kgdet_amd import evaluation as ev

FILL_SIM = np.array([0x7ff8badc0ffee000], dtype=np.uint64).view(np.float64)[0]        # a NaN no kernel computes
FILL_I32, FILL_U8 = -7, 0xEE
SIM_KS = [1, 63, 64, 65, 294]
MATCH_SHAPES = [(1, 1), (3, 10), (4, 10), (4, 16), (1, 64), (64, 1)]


def cell_valid(cell, nd, ng):
    d0, D, g0, G = (int(v) for v in cell)
    return d0 >= 0 and D >= 0 and g0 >= 0 and G >= 0 and d0 + D <= nd and g0 + G <= ng


def sim_valid(cell, off, sim_size):
    D, G = int(cell[1]), int(cell[3])
    return D > 0 and G > 0 and off >= 0 and off + D * G <= sim_size


# ------------------------------------------------------------------------------------------------------------ similarity cases
class _World(object):
    """detections and ground truths appended group by group, cells over them"""

    def __init__(self, K):
        self.K = K
        self.d_box, self.d_kxy, self.g_box, self.g_kpt, self.g_area, self.g_crowd = [], [], [], [], [], []
        self.cells, self.offs, self.size = [], [], 0

    def dets(self, boxes, kxy=None):
        boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
        first = len(self.d_box)
        for i, b in enumerate(boxes):
            self.d_box.append(b)
            self.d_kxy.append(np.zeros((self.K, 2)) if kxy is None else np.asarray(kxy[i], np.float64).reshape(self.K, 2))
        return first, len(boxes)

    def gts(self, boxes, kpt=None, area=None, crowd=None):
        boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
        first = len(self.g_box)
        for i, b in enumerate(boxes):
            self.g_box.append(b)
            self.g_kpt.append(np.zeros(3 * self.K) if kpt is None else np.asarray(kpt[i], np.float64).reshape(3 * self.K))
            self.g_area.append(float(b[2] * b[3]) if area is None else float(area[i]))
            self.g_crowd.append(0 if crowd is None else int(crowd[i]))
        return first, len(boxes)

    def cell(self, d, g, off='next', reserve=None):
        """a cell over (first, count) ranges; ``off``: 'next' = the next free block; ``reserve``: words of ``sim`` set aside for a
        cell that must be skipped (they have to keep their fill)"""
        n = d[1] * g[1] if reserve is None else reserve
        if off == 'next':
            off = self.size
            self.size += max(n, 0)
        self.cells.append((d[0], d[1], g[0], g[1]))
        self.offs.append(off)

    def finish(self, iou_type, order=None, tail_cell=None):
        if tail_cell is not None:                      # a cell ending ONE word past the matrix: off + D G = sim_size + 1
            d, g = tail_cell
            n = d[1] * g[1]
            self.cells.append((d[0], d[1], g[0], g[1]))
            self.offs.append(self.size + 1)
            self.size += n
        cells, offs = np.array(self.cells, np.int32).reshape(-1, 4), np.array(self.offs, np.int64)
        if order is not None:
            cells, offs = cells[order], offs[order]
        K = self.K
        g_kpt = np.array(self.g_kpt, np.float64).reshape(-1, 3 * K)
        sigmas = ev.landmark_meta()['oks_sigmas'][:K]
        return types.SimpleNamespace(
            iou_type=iou_type, K=K, cells=cells, sim_off=offs, sim_size=int(self.size), nd=len(self.d_box), ng=len(self.g_box),
            d_box=np.array(self.d_box, np.float64).reshape(-1, 4), d_kxy=np.array(self.d_kxy, np.float64).reshape(-1, K, 2),
            g_box=np.array(self.g_box, np.float64).reshape(-1, 4), g_kpt=g_kpt, g_area=np.array(self.g_area, np.float64),
            g_crowd=np.array(self.g_crowd, np.int32), g_nvis=(g_kpt[:, 2::3] > 0).sum(axis=1).astype(np.int32),
            sigmas=np.asarray(sigmas, np.float64), var=(np.asarray(sigmas, np.float64) * 2) ** 2)


def _skipped_cells(w, d, g):
    """the skip rules on valid-looking ranges ``d``, ``g`` ((first, count) each), every one with room in ``sim`` it must not use"""
    n = d[1] * g[1]
    w.cell((-1, d[1]), g, reserve=n)                                  # a negative start
    w.cell((len(w.d_box) - d[1] + 1, d[1]), g, reserve=n)             # one detection past ND
    w.cell(d, (len(w.g_box) - g[1] + 1, g[1]), reserve=n)             # one ground truth past NG
    w.cell(d, (g[0], -1), reserve=n)                                  # a negative count
    w.cell(d, g, off=-1)                                              # sim_off = -1


def iou_case():
    w = _World(1)
    rng = np.random.default_rng(11)
    # touching, zero / negative extents, identical, far coordinates
    d = w.dets([[10, 10, 20, 20], [30, 10, 5, 5], [10, 30, 20, 0], [0, 0, 0, 0], [40, 40, -10, 10], [50, 50, -5, -5],
                [12.5, 11.25, 7.5, 3.75], [1e8, 1e8, 16.5, 8.25], [1e8 + 8, 1e8 - 2, 16, 8]])
    g = w.gts([[10, 10, 20, 20], [30, 10, 20, 20], [10, 30, 20, 20], [12.5, 11.25, 7.5, 3.75], [0, 0, 0, 0], [35, 35, -10, 30],
               [1e8, 1e8, 16.5, 8.25], [5, 5, 100, 100], [5, 5, 100, 100]],
              crowd=[0, 0, 0, 0, 0, 0, 0, 1, 0])
    w.cell(d, g)
    # a crowd against detections of zero area, inside it and on its border
    d2 = w.dets([[20, 20, 0, 10], [20, 20, 10, 0], [5, 5, 0, 0], [20, 20, 4, 4]])
    g2 = w.gts([[5, 5, 100, 100], [5, 5, 100, 100]], crowd=[1, 0])
    w.cell(d2, g2)
    w.cell((d[0], 0), g2)                                             # D = 0
    w.cell(d2, (g[0], 0))                                             # G = 0
    w.cell((0, 0), (0, 0))                                            # both
    one_d, one_g = w.dets([[3, 4, 8, 6]]), w.gts([[5, 5, 8, 6]])
    w.cell(one_d, one_g)                                              # D G = 1
    xy = rng.integers(0, 200, (70, 2)) / 4.0
    wh = rng.integers(1, 160, (70, 2)) / 4.0
    big_d = w.dets(np.concatenate([xy, wh], axis=1))
    xy, wh = rng.integers(0, 200, (33, 2)) / 4.0, rng.integers(1, 160, (33, 2)) / 4.0
    big_g = w.gts(np.concatenate([xy, wh], axis=1), crowd=(np.arange(33) % 5 == 0).astype(int))
    w.cell(big_d, big_g)                                              # 2310 pairs: a workgroup takes ten trips
    _skipped_cells(w, d2, g2)
    n = len(w.cells)
    return w.finish('bbox', order=np.roll(np.arange(n + 1), 3)[::-1].copy(), tail_cell=(one_d, one_g))


def oks_case(K):
    w = _World(K)
    rng = np.random.default_rng(100 + K)

    def gt_kpt(n, vis):
        k = np.zeros((n, K, 3))
        k[..., :2] = rng.integers(160, 192, (n, K, 2)) / 4.0           # a grid of 1/4 inside [40, 48): arguments stay below 640
        k[..., 2] = vis
        return k

    # visibility 0, 1, 2 and negative; moderate distances: every exponent argument is 0 or within (0, 60)
    vis = np.stack([np.resize([2, 1, 0, -1, 2], K), np.resize([0, 0, 1], K), np.ones(K), np.resize([-1, 0, 2, 2], K)])
    vis[1, 0] = 1                                                     # (at least one labelled landmark per row)
    vis[3, -1] = 2
    gk = gt_kpt(4, vis)
    g = w.gts([[10, 10, 80, 80]] * 4, kpt=gk.reshape(4, -1), area=[6400.0, 3000.5, 812.25, 6400.0])
    sd = np.sqrt(w.g_area[g[0] + 2]) * 0.05
    dk = np.stack([gk[0, :, :2], gk[1, :, :2] + rng.normal(0, sd, (K, 2)), gk[2, :, :2] + rng.normal(0, sd, (K, 2)),
                   gk[3, :, :2] + rng.normal(0, 2 * sd, (K, 2)), gk[0, :, :2] + 0.25])
    d = w.dets([[0, 0, 1, 1]] * 5, kxy=dk)
    w.cell(d, g)
    # no labelled landmark (g_nvis = 0): the doubled box [bx - bw, bx + 2 bw]; points inside, outside, exactly on it
    gb = [[40, 40, 20, 10], [40, 40, 20, 10]]
    g0 = w.gts(gb, kpt=gt_kpt(2, 0).reshape(2, -1), area=[200.0, 800.0])
    inside = np.stack([rng.integers(80, 320, K) / 4.0, rng.integers(120, 240, K) / 4.0], axis=1)         # x [20, 80], y [30, 60]
    on = np.stack([np.resize([20.0, 80.0, 50.0], K), np.resize([30.0, 60.0], K)], axis=1)
    out = on + np.stack([np.resize([-6.0, 6.0, 0.0], K), np.resize([-3.0, 6.0], K)], axis=1)
    near = on + np.stack([np.resize([-1.5, 1.5, 0.0], K), np.resize([-0.75, 2.25], K)], axis=1)
    d0 = w.dets([[0, 0, 1, 1]] * 4, kxy=np.stack([inside, on, out, near]))
    w.cell(d0, g0)
    # area 0: the argument is 0 where the landmark coincides and overflows where it does not -> terms exactly 1 and 0
    ga = gt_kpt(1, np.resize([2, 1], K))
    g_zero = w.gts([[10, 10, 80, 80]], kpt=ga.reshape(1, -1), area=[0.0])
    moved = ga[0, :, :2].copy()
    moved[::2] += 0.25
    far = ga[0, :, :2] + 1e4
    d_zero = w.dets([[0, 0, 1, 1]] * 3, kxy=np.stack([ga[0, :, :2], moved, far]))
    w.cell(d_zero, g_zero)
    # every argument above 746: exactly 0.0 (labelled and unlabelled ground truth)
    d_far = w.dets([[0, 0, 1, 1]], kxy=(gk[0, :, :2] + 3e5)[None])
    w.cell(d_far, (g[0], 1))
    w.cell(d_far, (g0[0], 1))
    w.cell((d[0], 0), g)                                              # D = 0
    w.cell(d, (g[0], 0))                                              # G = 0
    w.cell((0, 0), (0, 0))
    w.cell((d[0] + 1, 1), (g[0] + 1, 1))                              # D G = 1
    if K in (1, 65):
        gk2 = gt_kpt(33, rng.integers(-1, 3, (33, K)))
        gk2[:, 0, 2] = 2
        gk2[5, :, 2] = 0                                              # (one of the 33 without a labelled landmark)
        big_g = w.gts(np.concatenate([rng.integers(40, 200, (33, 2)) / 4.0, rng.integers(40, 200, (33, 2)) / 4.0], axis=1),
                      kpt=gk2.reshape(33, -1), area=rng.integers(400, 8000, 33) + 0.5)
        big_d = w.dets([[0, 0, 1, 1]] * 70, kxy=gk2[rng.integers(0, 33, 70), :, :2] + rng.normal(0, 1.5, (70, K, 2)))
        w.cell(big_d, big_g)                                          # 2310 pairs over the four waves of a workgroup
    _skipped_cells(w, d0, g0)
    n = len(w.cells)
    return w.finish('keypoints', order=np.roll(np.arange(n + 1), 5)[::-1].copy(), tail_cell=((d[0], 1), (g[0], 1)))


def sim_case(name):
    return iou_case() if name == 'iou' else oks_case(int(name[3:]))


SIM_NAMES = ['iou'] + ['oks%d' % K for K in SIM_KS]


def reference_similarity(c):
    """``sim`` [sim_size] starting at FILL_SIM: evaluation.box_iou_xywh / evaluation.oks on every cell the kernels take"""
    sim = np.full(c.sim_size, FILL_SIM)
    for cell, off in zip(c.cells, c.sim_off):
        if not (cell_valid(cell, c.nd, c.ng) and sim_valid(cell, int(off), c.sim_size)):
            continue
        d0, D, g0, G = (int(v) for v in cell)
        if c.iou_type == 'bbox':
            block = ev.box_iou_xywh(c.d_box[d0:d0 + D], c.g_box[g0:g0 + G], c.g_crowd[g0:g0 + G])
        else:
            dts = np.concatenate([c.d_kxy[d0:d0 + D], np.ones((D, c.K, 1))], axis=2).reshape(D, -1)
            gts = [dict(keypoints=c.g_kpt[j], bbox=list(c.g_box[j]), area=c.g_area[j]) for j in range(g0, g0 + G)]
            block = ev.oks(dts, gts, c.sigmas)
        sim[off:off + D * G] = np.asarray(block, np.float64).reshape(-1)
    return sim


def oks_arguments(c):
    """per valid cell: (offset, [D, G] masks 'every exponent argument is 0' / 'every argument is above 746', the number of
    pairs whose SMALLEST argument lies in (640, 746]) -- the similarities that are exactly 1.0 / 0.0 in any correct exp and any
    summation order (exp(-746) is below half the smallest subnormal), and a count that must be 0: a similarity below ~1e-278
    is a sum of results of exp in or next to the subnormal range, which carry no relative accuracy in any library, so the
    cases keep out of it (a subnormal TERM beside larger ones is harmless: its absolute error is below 5e-324)"""
    out = []
    for cell, off in zip(c.cells, c.sim_off):
        if not (cell_valid(cell, c.nd, c.ng) and sim_valid(cell, int(off), c.sim_size)):
            continue
        d0, D, g0, G = (int(v) for v in cell)
        ones, zeros, risky = np.zeros((D, G), bool), np.zeros((D, G), bool), 0
        for j in range(G):
            k = c.g_kpt[g0 + j].reshape(c.K, 3)
            vis = k[:, 2] > 0
            for i in range(D):
                xd, yd = c.d_kxy[d0 + i, :, 0], c.d_kxy[d0 + i, :, 1]
                if vis.any():
                    dx, dy = (xd - k[:, 0])[vis], (yd - k[:, 1])[vis]
                    var = c.var[vis]
                else:
                    bx, by, bw, bh = c.g_box[g0 + j]
                    dx = np.maximum(0, (bx - bw) - xd) + np.maximum(0, xd - (bx + bw * 2))
                    dy = np.maximum(0, (by - bh) - yd) + np.maximum(0, yd - (by + bh * 2))
                    var = c.var
                with np.errstate(over='ignore'):
                    e = (dx ** 2 + dy ** 2) / var / (c.g_area[g0 + j] + np.spacing(1)) / 2
                ones[i, j], zeros[i, j] = bool((e == 0).all()), bool((e > 746).all())
                risky += int(640 < e.min() <= 746)
        out.append((int(off), ones, zeros, risky))
    return out


# --------------------------------------------------------------------------------------------------------------- matching cases
def _thresholds(T):
    if T == 10:
        return np.linspace(0.5, 0.95, 10)                             # EvalParams.iou_thrs
    if T == 1:
        return np.array([0.5])
    return np.arange(1, T + 1) / float(T)                             # a dyadic grid up to 1.0 (capped at 1 - 1e-10 below)


def _area_ranges(A):
    if A == 1:
        return np.array([[0, 1e10]])
    if A == 3:
        return np.array([[0, 1e10], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], np.float64)
    if A == 4:
        return np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], np.float64)
    base = _area_ranges(4)
    return np.array([[base[a % 4, 0] + 16 * (a // 4) * (a % 4 in (2, 3)), base[a % 4, 1] - 16 * (a // 4) * (a % 4 in (1, 2))]
                     for a in range(A)], np.float64)


def match_case(A, T, thresholds=None):
    """one chunk with every rule of the matcher in a cell of its own (names in ``c.cell_names``); rows of different cells are
    disjoint, rows of skipped cells belong to nobody else"""
    thr = _thresholds(T) if thresholds is None else np.asarray(thresholds, np.float64)
    best0 = np.minimum(thr, 1 - 1e-10)
    tq = T // 2
    on, below = best0[tq], np.nextafter(best0[tq], 0.0)
    rows = dict(d_area=[], g_area=[], g_ign=[], g_crowd=[])
    cells, offs, sims, names = [], [], [], []
    size = [0]

    def add(name, d_area, g, sim=None, off='next', valid=True, shift=(0, 0)):
        """g: [(area, ignore flag, crowd)]; sim [D, G] or None; ``shift``: moves the cell's starts (for the skipped ones)"""
        d0, g0 = len(rows['d_area']), len(rows['g_area'])
        rows['d_area'] += list(d_area)
        for area, ign, crowd in g:
            rows['g_area'].append(area); rows['g_ign'].append(ign); rows['g_crowd'].append(crowd)
        D, G = len(d_area), len(g)
        if off == 'next':
            off = size[0]
            block = np.full(D * G, 0.0) if sim is None else np.asarray(sim, np.float64).reshape(D * G)
            sims.append(block)
            size[0] += D * G
        cells.append((d0 + shift[0], D, g0 + shift[1], G))
        offs.append(off)
        names.append(name)

    M, S, L = 2000.0, 100.0, 20000.0                                 # medium, small, large areas
    add('threshold', [M, M, M, M], [(M, 0, 0)] * 4,
        [[on, 0, 0, 0], [0, below, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 0.015625]])
    add('ties', [M, M, M], [(M, 0, 0), (M, 0, 0)], [[0.75, 0.75], [0.75, 0.75], [0.75, 0.75]])
    add('ties3', [M, M], [(M, 0, 0), (M, 0, 0), (M, 0, 0)], [[0.5, 0.875, 0.875], [0.875, 0.5, 0.875]])
    add('ignored_first', [M, M], [(M, 1, 0), (M, 0, 0), (S, 0, 0), (L, 0, 0)],
        [[0.875, 0.625, 0.75, 0.6875], [0.875, 0.625, 0.75, 0.6875]])
    add('gt_areas_on_borders', [M, M, M, M, M, M],
        [(1024.0, 0, 0), (9216.0, 0, 0), (np.nextafter(1024.0, 0), 0, 0), (np.nextafter(9216.0, 1e9), 0, 0), (0.0, 0, 0), (1e10, 0, 0)],
        np.eye(6) * 0.984375)
    add('det_areas_on_borders', [1024.0, 9216.0, np.nextafter(1024.0, 0), np.nextafter(9216.0, 1e9), 0.0, 1e10, 1e11],
        [(M, 0, 0)], np.zeros((7, 1)))
    add('crowd_reused', [M, S, L, M], [(M, 1, 1), (M, 0, 0)], [[0.75, 0.0], [0.75, 0.0], [0.75, 0.0], [0.75, 0.75]])
    add('regular_once', [M, M, M], [(M, 0, 0)], [[0.96875], [0.96875], [1.0]])
    add('low_thresholds_only', [M, M], [(M, 0, 0), (M, 0, 0)], [[0.625, 0.5], [0.75, 0.5]])
    add('ignored_not_crowd_once', [M, M], [(M, 1, 0)], [[0.875], [0.875]])
    add('no_ground_truth', [M, S, 1024.0], [])
    add('no_detection', [], [(M, 0, 0), (S, 0, 0), (1024.0, 1, 0), (9216.0, 0, 1)])
    add('nan_similarity', [M, M], [(M, 0, 0), (M, 0, 0), (M, 0, 0)], [[0.25, np.nan, 0.125], [1.0, 0.0, 0.0]])
    add('sim_off_negative', [M, S], [(M, 0, 0), (S, 0, 0)], off=-1)
    add('skipped_negative_start', [M, M], [(M, 0, 0)], [[1.0], [1.0]], shift=(-len(rows['d_area']) - 1, 0))
    add('sim_off_past_the_end', [L, 1024.0], [(M, 0, 0), (L, 1, 0)], off='tail')
    add('skipped_past_NG', [M], [(M, 0, 0), (M, 0, 0)], [[1.0, 1.0]], shift=(0, 1))          # (the last ground-truth rows)
    add('skipped_past_ND', [M, M], [], shift=(1, 0))                                          # (the last detection rows)
    sim = np.concatenate(sims) if sims else np.zeros(0)
    offs = [len(sim) - 4 + 1 if o == 'tail' else o for o in offs]    # 2 x 2 words needed, three left: off + D G = sim_size + 1
    order = np.roll(np.arange(len(cells)), 4)                         # listed out of array order
    return types.SimpleNamespace(
        A=A, T=T, cells=np.array(cells, np.int32)[order], sim_off=np.array(offs, np.int64)[order], cell_names=[names[i] for i in order],
        sim=sim, sim_size=len(sim), nd=len(rows['d_area']), ng=len(rows['g_area']),
        d_area=np.array(rows['d_area'], np.float64), g_area=np.array(rows['g_area'], np.float64),
        g_ign=np.array(rows['g_ign'], np.uint8), g_crowd=np.array(rows['g_crowd'], np.int32),
        area_rng=_area_ranges(A), best0=best0, thr=thr, tq=tq)


def reference_match(c, sim=None):
    """(d_match [ND, A, T] int32: ground-truth row + 1 or 0, d_ignore [ND, A, T] uint8, g_ignore [NG, A] uint8), rows of no valid
    cell left at FILL_I32 / FILL_U8.  One scalar loop per lane, from ``CocoEvaluator._match``."""
    sim = c.sim if sim is None else sim
    A, T = len(c.area_rng), len(c.best0)
    d_match = np.full((c.nd, A, T), FILL_I32, np.int32)
    d_ignore = np.full((c.nd, A, T), FILL_U8, np.uint8)
    g_out = np.full((c.ng, A), FILL_U8, np.uint8)
    for cell, off in zip(c.cells, c.sim_off):
        if not cell_valid(cell, c.nd, c.ng):
            continue
        d0, D, g0, G = (int(v) for v in cell)
        block = sim[off:off + D * G].reshape(D, G) if sim_valid(cell, int(off), c.sim_size) else None
        for a, (lo, hi) in enumerate(c.area_rng):
            g_ign = np.array([int(bool(c.g_ign[g0 + j]) or c.g_area[g0 + j] < lo or c.g_area[g0 + j] > hi) for j in range(G)], np.int64)
            g_out[g0:g0 + G, a] = g_ign
            order = np.argsort(g_ign, kind='mergesort')               # regular ground truths first, each group in its order
            for t in range(T):
                taken = np.zeros(G, bool)
                for di in range(D):
                    best, m = c.best0[t], -1
                    if block is not None:
                        for j in order:
                            if taken[j] and not c.g_crowd[g0 + j]:
                                continue
                            if m > -1 and g_ign[m] == 0 and g_ign[j] == 1:
                                break                                 # a regular match exists and only ignore regions follow
                            if block[di, j] < best:
                                continue
                            best, m = block[di, j], j
                    if m >= 0:
                        taken[m] = True
                        d_match[d0 + di, a, t] = g0 + m + 1
                        d_ignore[d0 + di, a, t] = g_ign[m]
                    else:
                        da = c.d_area[d0 + di]
                        d_match[d0 + di, a, t] = 0
                        d_ignore[d0 + di, a, t] = int(da < lo or da > hi)
    return d_match, d_ignore, g_out


def cell_of(c, name):
    i = c.cell_names.index(name)
    return tuple(int(v) for v in c.cells[i])


def in_domain(c, sim):
    """the same chunk inside the domain of ``evaluation_device.match_restatement`` (which indexes without checks): cells the
    kernels skip are dropped, a cell without similarities gets a block of -1 (below every threshold: nothing matches)"""
    cells, offs, extra = [], [], []
    size = c.sim_size
    for cell, off in zip(c.cells, c.sim_off):
        if not cell_valid(cell, c.nd, c.ng):
            continue
        D, G = int(cell[1]), int(cell[3])
        if D > 0 and G > 0 and not sim_valid(cell, int(off), c.sim_size):
            off = size
            extra.append(np.full(D * G, -1.0))
            size += D * G
        cells.append(cell)
        offs.append(off)
    out = types.SimpleNamespace(**vars(c))
    out.cells, out.sim_off = np.array(cells, np.int32).reshape(-1, 4), np.array(offs, np.int64)
    full = np.concatenate([sim] + extra)
    out.sim, out.sim_size = full, len(full)
    return out, full


def written_rows(c):
    """(detection rows, ground-truth rows) some valid cell owns"""
    d, g = np.zeros(c.nd, bool), np.zeros(c.ng, bool)
    for cell in c.cells:
        if cell_valid(cell, c.nd, c.ng):
            d[cell[0]:cell[0] + cell[1]] = True
            g[cell[2]:cell[2] + cell[3]] = True
    return d, g
