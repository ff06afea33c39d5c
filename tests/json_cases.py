"""Inputs shared by tests/test_json_refs.py (numpy) and tests/test_gpu_json_out.py (HIP kernels): the detections of a test run
as ``runner.DeviceResults.rows`` holds them -- float32 [N, M, 7 + 3K]: box, score, label, count, landmarks -- with the
dataset stub the result writers read (``img_ids``, ``cat_ids``, ``__len__``; no annotations).  Seeds are fixed.

Sizes: N = 5 images of M = 7 rows; K = 1, 22, 294 landmarks = 3, 66, 882 values per record: under a wave of the measure
kernel, one trip plus two lanes, 13 trips plus 50.  Every generated case: an image with count 0, images whose rows are not in
label order, labels of -1 and L (dropped), counts below M with NaN / 2^40 in the rows beyond the count, the edge values
sprinkled over boxes, scores and landmarks.  ``edge`` is hand-made: every edge value at every landmark position, as x1, y1
and score, and boxes with x2 < x1."""
import numpy as np

from kgdet_amd import evaluation as ev

N, M = 5, 7
# (the last one is the largest float32 below 2^40 / 10^4; 1099511.5 * 10^4 needs 34 bits)
EDGE = np.array([0.0, -0.0, -1e-5, 4.9e-5, 5e-5, 1e-4, 1.5, 1.25, 12.0, 0.99996, -123.45675, 1099511.5, 109951160.0], np.float32)
# landmark values outside the domain: the last is the smallest float32 at or above 2^40 / 10^4 (= 109951162.7776)
OUTSIDE = [np.float32(np.nan), np.float32(np.inf), np.float32(109951168.0)]
IMG_IDS = [0, 7, 123456, 2 ** 40, 99]
CATS_13 = list(range(1, 14))
CATS_SPARSE = [3, 50, 7, 2 ** 40 + 5]
NAMES = ['k1', 'k22', 'k294', 'edge']


class Dataset(object):
    """all the result writers read of a dataset"""

    def __init__(self, img_ids, cat_ids):
        self.img_ids, self.cat_ids = list(img_ids), list(cat_ids)

    def __len__(self):
        return len(self.img_ids)


class Case(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _spread(rng, shape, top):
    """float32 values spread over the decades from 1e-6 up to ``top``, both signs"""
    v = 10.0 ** rng.uniform(-6, np.log10(top), shape) * rng.choice([-1.0, 1.0], shape)
    return v.astype(np.float32)


def _generated(seed, K, L):
    rng = np.random.default_rng(seed)
    rows = np.full((N, M, 7 + 3 * K), np.nan, np.float32)
    counts = [7, 0, 5, 3, 7]
    for n, c in enumerate(counts):
        x1, y1 = rng.uniform(0, 400, c), rng.uniform(0, 300, c)
        rows[n, :c, 0], rows[n, :c, 1] = x1, y1
        rows[n, :c, 2], rows[n, :c, 3] = x1 + rng.uniform(5, 200, c), y1 + rng.uniform(5, 150, c)
        rows[n, :c, 4] = rng.random(c)
        rows[n, :c, 5] = rng.integers(0, L, c)
        kp = _spread(rng, (c, 3 * K), 1e5)
        pick = rng.random((c, 3 * K)) < 0.15
        kp[pick] = EDGE[rng.integers(0, len(EDGE), int(pick.sum()))]
        rows[n, :c, 7:] = kp
        for col in (0, 1, 4):                                       # edge values as x1, y1 and score of some rows
            pick = rng.random(c) < 0.3
            rows[n, :c, col][pick] = EDGE[rng.integers(0, len(EDGE), int(pick.sum()))]
        rows[n, c:, :] = np.where(np.arange(M - c)[:, None] % 2 == 0, np.float32(np.nan), np.float32(2.0 ** 40))
        rows[n, :, 6] = np.nan
        rows[n, 0, 6] = c
    rows[0, :7, 5] = np.array([3, 1, 0, 2, 1, 3, 0]) % L            # not in label order
    rows[4, :7, 5] = np.arange(7)[::-1] % L                         # descending
    rows[2, 1, 5], rows[2, 3, 5] = -1, L                            # dropped
    rows[3, 0, 2] = rows[3, 0, 0] - 37.25                           # x2 < x1: a negative width
    return rows


def _edge(K=5, L=13):
    rows = np.full((N, M, 7 + 3 * K), np.nan, np.float32)
    pad = np.concatenate([EDGE, EDGE[:3 * K - len(EDGE)]])
    for n in range(N):
        c = [7, 7, 0, 6, 1][n]
        for i in range(c):
            j = n * M + i
            rows[n, i, 7:] = np.roll(pad, j)
            rows[n, i, 0], rows[n, i, 1] = EDGE[j % len(EDGE)], EDGE[(j + 5) % len(EDGE)]
            rows[n, i, 2] = rows[n, i, 0] + (10.5 if j % 2 else -3.25)        # (odd j: a width of 11.5; even: x2 < x1)
            rows[n, i, 3] = rows[n, i, 1] + 1.0
            rows[n, i, 4] = EDGE[(j + 2) % len(EDGE)]
            rows[n, i, 5] = (j * 5) % L
        rows[n, c:, :] = np.float32(2.0 ** 40)
        rows[n, 0, 6] = c
    return rows


_cache = {}


def case(name):
    """-> Case(name, dataset, rows [N, M, 7 + 3K] float32, K, n_labels); built once, leave unchanged"""
    if name not in _cache:
        if name == 'edge':
            K, cats, rows = 5, CATS_13, _edge()
        else:
            K = int(name[1:])
            cats = CATS_SPARSE if K == 22 else CATS_13
            rows = _generated(200 + K, K, len(cats))
        _cache[name] = Case(name=name, dataset=Dataset(IMG_IDS, cats), rows=rows, K=K, n_labels=len(cats))
    return _cache[name]


def empty_case(K=3):
    rows = np.full((2, M, 7 + 3 * K), np.nan, np.float32)
    rows[:, 0, 6] = 0
    return Case(name='empty', dataset=Dataset(IMG_IDS[:2], CATS_13), rows=rows, K=K, n_labels=13)


def host_results(c, rows=None):
    """the list ``runner.DeviceResults.to_host()`` makes of the rows, built with ``evaluation.detections2result`` per image"""
    rows = c.rows if rows is None else rows
    out = []
    for n in range(rows.shape[0]):
        cnt = int(rows[n, 0, 6])
        r = rows[n, :cnt]
        if cnt == 0:                                                # (bbox2result_kp's 1-tuple for an image without detections)
            out.append(([np.zeros((0, 5), np.float32) for _ in range(c.n_labels)],))
            continue
        out.append(ev.detections2result(r[:, :5].copy(), r[:, 5].astype(np.int64), r[:, 7:], c.n_labels + 1))
    return out


def formatter_values(num_digits, n=20000, seed=7):
    """float32 values over the decades of the domain ``|v| * 10**d < 2**40``, both signs, and the edge set"""
    rng = np.random.default_rng(seed + num_digits)
    v = _spread(rng, n, 2.0 ** 40 / 10.0 ** num_digits)
    v = np.concatenate([v, EDGE, -EDGE]).astype(np.float32)
    return v[np.abs(v.astype(np.float64)) * 10.0 ** num_digits < 2.0 ** 40]
