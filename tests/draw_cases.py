"""Shared by tests/test_draw_refs.py, tests/test_gpu_draw.py and tests/test_gpu_show.py: seeded images and row blocks in the
layout of ``decode.pack_rows`` (box 4, score, label, count, K x (x, y, v)) for ``visualize.draw_restatement`` and
``kgdet_draw_detections``.  Nothing here is committed data."""
import numpy as np

NAMES3 = ['top', 'long sleeve_dress', 'Sk-1.x']          # (lower and upper case, space, '_', '-', '.', digits)
TWO40 = float(2 ** 40)


def image(H, W, seed=0):
    return np.random.default_rng(1000 + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def empty_rows(M, K):
    return np.zeros((M, 7 + 3 * K), dtype=np.float32)


def set_row(rows, r, box, score, label, pts=None):
    rows[r, :4], rows[r, 4], rows[r, 5] = box, score, label
    if pts is not None:
        pts = np.asarray(pts, dtype=np.float32).reshape(-1)
        rows[r, 7:7 + len(pts)] = pts


def finish(rows, count):
    """the count in column 6; rows at and beyond it hold NaN and 2^40 and must leave no trace"""
    rows[count:, 0::2] = np.nan
    rows[count:, 1::2] = TWO40
    rows[:, 6] = count
    return rows


def random_rows(seed, M, K, H, W, L, count=None, visible=0.8):
    """boxes around and partly outside the image, scores on both sides of 0.3, landmarks scattered about their box with
    fractional coordinates (halves among them: rint's ties)"""
    rng = np.random.default_rng(seed)
    count = M if count is None else count
    rows = empty_rows(M, K)
    cx, cy = rng.uniform(-0.2 * W, 1.2 * W, M), rng.uniform(-0.2 * H, 1.2 * H, M)
    bw, bh = rng.uniform(0, 0.7 * W + 4, M), rng.uniform(0, 0.7 * H + 4, M)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2
    rows[:, :4] = np.round(rows[:, :4] * 2) / 2
    rows[:, 4] = rng.uniform(0.05, 1.0, M)
    rows[:, 5] = rng.integers(0, L, M)
    pts = rows[:, 7:].reshape(M, K, 3)
    pts[..., 0] = np.round((cx[:, None] + rng.uniform(-0.6, 0.6, (M, K)) * (bw[:, None] + 6)) * 4) / 4
    pts[..., 1] = np.round((cy[:, None] + rng.uniform(-0.6, 0.6, (M, K)) * (bh[:, None] + 6)) * 4) / 4
    pts[..., 2] = np.where(rng.uniform(0, 1, (M, K)) < visible, rng.choice([1.0, 2.0, 0.7], (M, K)), 0.0)
    return finish(rows, count)


def awkward_rows(M, H, W, L, count):
    """``random_rows`` (K = 3) with the rows that must draw nothing, or less, mixed in where the count allows"""
    rows = random_rows(7 * M + count, M, 3, H, W, L, count=count)
    specials = [
        lambda r: rows.__setitem__((r, 1), np.nan),              # a NaN box value: the whole row draws nothing
        lambda r: rows.__setitem__((r, 7 + 3), np.nan),          # a NaN landmark x: that landmark alone is skipped
        lambda r: rows.__setitem__((r, 5), -1.0),
        lambda r: rows.__setitem__((r, 5), float(L)),
        lambda r: rows.__setitem__((r, 5), 2.5),
        lambda r: rows.__setitem__((r, 4), np.float32(0.3)),     # exactly at the threshold: mmcv's strict >
        lambda r: rows.__setitem__((r, 2), np.inf),
        lambda r: rows.__setitem__((r, 4), np.nan),
    ]
    for k, make in enumerate(specials):
        r = 2 * k + 1
        if r < count:
            rows[r, 4] = 0.9
            rows[r, 9::3] = 1.0
            make(r)
    return rows


def box_rows(H, W):
    """boxes wholly inside, straddling each edge, wholly outside, one pixel wide, empty, thinner than 2t (filled for t = 2),
    coordinates at +-1e9 (clamped)"""
    boxes = [
        (10, 12, 50, 40), (70, 20, 90, 60),                                   # inside (two tiles apart in x and y)
        (-9, 5, 12, 30), (W - 8, 3, W + 20, 25), (20, -7, 44, 6), (30, H - 5, 61, H + 9),     # straddling each edge
        (-50, -50, -3, -2), (W + 1, 4, W + 30, 9), (3, H, 9, H + 4),          # wholly outside
        (33, 44, 33, 60), (40, 50, 70, 50), (5, 5, 5, 5),                     # one pixel wide / tall / a single pixel
        (60, 30, 59, 40), (20, 41, 30, 40),                                   # empty
        (63, 14, 65, 17), (15, 60, 17, 62), (80, 5, 82, 30),                  # thinner than 2t
        (-1e9, 35, 1e9, 45), (50, -1e9, 56, 1e9), (-1e9, -1e9, 1e9, 1e9),     # clamped
        (62.5, 14.5, 66.5, 17.5), (0.49999, 0.5, 1.5, 2.5),                   # ties of rint: half to even
    ]
    rows = empty_rows(len(boxes) + 2, 3)
    for r, b in enumerate(boxes):
        set_row(rows, r, b, 0.31 + 0.03 * r, r % 3)                           # (no landmark is visible)
    return finish(rows, len(boxes))


def landmark_rows(H, W):
    """K = 3: discs and segments across tile borders (x = 64, y = 16, 32, ...) and image edges; a contour broken by an
    invisible landmark; a horizontal, a vertical and a zero-length segment; a NaN landmark; far-away landmarks"""
    rows = empty_rows(10, 3)
    set_row(rows, 0, (40, 8, 90, 40), 0.9, 0, [(63.5, 15.5, 1), (64.5, 16.5, 2), (20, 33, 1)])
    set_row(rows, 1, (2, 2, 30, 30), 0.8, 1, [(0, 0, 1), (W - 1, 1, 0), (W - 1, H - 1, 1)])      # broken in the middle
    set_row(rows, 2, (10, 40, 95, 60), 0.7, 2, [(5, 50, 1), (97, 50, 1), (97, 69, 1)])            # horizontal, vertical
    set_row(rows, 3, (50, 20, 80, 50), 0.6, 0, [(70, 30, 1), (70, 30, 1), (-3, H + 2, 1)])        # zero length, off-image
    set_row(rows, 4, (5, 45, 40, 65), 0.5, 1, [(12, 55, np.nan), (np.nan, 55, 1), (30, np.inf, 1)])
    set_row(rows, 5, (60, 40, 99, 69), 0.95, 2, [(-1e9, -1e9, 1), (1e9, 1e9, 1), (80, 1e9, 1)])   # clamped, a long diagonal
    set_row(rows, 6, (20, 5, 60, 25), 0.4, 0, [(31.25, 9.75, 1), (47.5, 20.5, 1), (58.5, 6.5, 0.001)])
    return finish(rows, 7)
