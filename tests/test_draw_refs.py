"""``visualize.draw_restatement`` -- the definition of the picture and the yardstick of ``kgdet_draw_detections`` -- pinned to
independent formulations: PIL's rectangle, float64 distances, exact Python integers, ``'%.2f'``."""
import math

import numpy as np
import pytest

from kgdet_amd import visualize as vz
from tests import demo_checks
from tests import draw_cases as dc
from tests.golden import demo_cases

GREY = 90
FAR = (-5000, -5000, -4000, -4000)                      # a box (and its label) nowhere near the image


def _plain(H, W):
    return np.full((H, W, 3), GREY, dtype=np.uint8)


def _label_rect(x0, y0, name, s=1):
    """(left, top, right, bottom), inclusive, of the text box of ``name|d.dd``"""
    top = y0 - 9 * s if y0 - 9 * s >= 0 else y0
    return x0, top, x0 + (6 * (len(name) + 5) + 1) * s - 1, top + 9 * s - 1


def test_box_layer_equals_pil_rectangle():
    from PIL import Image, ImageDraw
    rng = np.random.default_rng(5)
    H, W = 60, 90
    colour = tuple(int(c) for c in vz.palette(1)[0])
    for case in range(300):
        t = int(rng.integers(1, 6))
        x0, y0 = int(rng.integers(-20, W)), int(rng.integers(-20, H))
        x1, y1 = x0 + int(rng.integers(2 * t, 70)), y0 + int(rng.integers(2 * t, 50))
        rows = dc.empty_rows(1, 1)
        dc.set_row(rows, 0, (x0, y0, x1, y1), 0.9, 0)
        got = vz.draw_restatement(_plain(H, W), rows, 1, ['a'], thickness=t)
        im = Image.fromarray(_plain(H, W))
        ImageDraw.Draw(im).rectangle([x0, y0, x1, y1], outline=colour, width=t)
        want = np.array(im)
        lx0, ly0, lx1, ly1 = _label_rect(x0, y0, 'a')
        yy, xx = np.mgrid[0:H, 0:W]
        outside_label = ~((xx >= lx0) & (xx <= lx1) & (yy >= ly0) & (yy <= ly1))
        assert np.array_equal(got[outside_label], want[outside_label]), (case, t, x0, y0, x1, y1)


def _covered(out):
    return (out != GREY).any(axis=2)


def test_discs_equal_a_float64_distance():
    """d^2 is an integer, so d^2 <= r^2 is d < sqrt(r^2 + 1/2): no pixel centre lies near that boundary"""
    rng = np.random.default_rng(6)
    H, W = 50, 70
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for case in range(60):
        r = int(rng.choice([1, 2, 3, 5, 13, 64]))
        cx, cy = rng.uniform(-10, W + 10), rng.uniform(-10, H + 10)
        rows = dc.empty_rows(1, 1)
        dc.set_row(rows, 0, FAR, 0.9, 0, [(cx, cy, 1)])
        got = _covered(vz.draw_restatement(_plain(H, W), rows, 1, ['a'], radius=r))
        ix, iy = float(np.rint(np.float32(cx))), float(np.rint(np.float32(cy)))
        dist = np.hypot(xx - ix, yy - iy)
        bound = math.sqrt(r * r + 0.5)
        assert np.abs(dist - bound).min() > 1e-6
        assert np.array_equal(got, dist < bound), (case, r, cx, cy)


def _segment_distance(xx, yy, px, py, qx, qy):
    dx, dy = qx - px, qy - py
    dd = dx * dx + dy * dy
    u = np.zeros_like(xx) if dd == 0 else np.clip(((xx - px) * dx + (yy - py) * dy) / dd, 0.0, 1.0)
    return np.hypot(xx - (px + u * dx), yy - (py + u * dy))


def test_capsules_equal_a_float64_distance():
    rng = np.random.default_rng(7)
    H, W = 50, 70
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    checked = 0
    for case in range(200):
        lw = int(rng.choice([1, 2, 3, 5, 16]))
        px, py, qx, qy = (int(v) for v in rng.integers(-15, 85, 4))
        dist = _segment_distance(xx, yy, px, py, qx, qy)
        if np.abs(dist - lw / 2.0).min() <= 1e-6:       # a pixel centre on the boundary: left to the exact test below
            continue
        rows = dc.empty_rows(1, 2)
        dc.set_row(rows, 0, FAR, 0.9, 0, [(px, py, 1), (qx, qy, 1)])
        got = _covered(vz.draw_restatement(_plain(H, W), rows, 1, ['a'], radius=1, line_width=lw, contour=True, kpt_color=None))
        discs = (np.hypot(xx - px, yy - py) < 1.2) | (np.hypot(xx - qx, yy - qy) < 1.2)      # (radius 1: the centre and its 4 neighbours)
        assert np.array_equal(got, (dist < lw / 2.0) | discs), (case, lw, px, py, qx, qy)
        checked += 1
    assert checked > 100


def _exact_capsule(x, y, px, py, qx, qy, lw):
    """the definition in Python integers (no width to overflow)"""
    X, Y, dx, dy = 2 * x, 2 * y, 2 * (qx - px), 2 * (qy - py)
    vx, vy, R2 = X - 2 * px, Y - 2 * py, lw * lw
    dot, dd = vx * dx + vy * dy, dx * dx + dy * dy
    if dot <= 0:
        return vx * vx + vy * vy <= R2
    if dot >= dd:
        return (X - 2 * qx) ** 2 + (Y - 2 * qy) ** 2 <= R2
    return (vx * dy - vy * dx) ** 2 <= R2 * dd


@pytest.mark.parametrize('lw', [1, 16])
def test_capsules_at_the_coordinate_clamps_equal_exact_integers(lw):
    """an 8192-wide strip, segments between the clamps -8192 / 16383 (given as +-1e9): cross^2 reaches 2^61 there, and an
    int64 overflow anywhere in the test would show against Python's integers"""
    H, W = 3, 8192
    lo, hi = vz.COORD_MIN, vz.COORD_MAX
    segments = [((-1e9, -1e9), (1e9, 1e9)), ((-1e9, 1e9), (1e9, -1e9)), ((-1e9, 1), (1e9, 1)), ((-1e9, -1e9), (1e9, 8194)),
                ((8191, -1e9), (8190, 1e9)), ((1e9, -1e9), (-1e9, 8194))]
    for p, q in segments:
        rows = dc.empty_rows(1, 2)
        dc.set_row(rows, 0, FAR, 0.9, 0, [p + (1,), q + (1,)])
        got = _covered(vz.draw_restatement(_plain(H, W), rows, 1, ['a'], radius=1, line_width=lw, contour=True, kpt_color=None))
        px, py, qx, qy = (int(min(max(v, lo), hi)) for v in p + q)
        want = np.array([[_exact_capsule(x, y, px, py, qx, qy, lw) or (x - px) ** 2 + (y - py) ** 2 <= 1
                          or (x - qx) ** 2 + (y - qy) ** 2 <= 1 for x in range(W)] for y in range(H)])
        assert want.any() and np.array_equal(got, want), (p, q)


def test_label_digits_equal_percent_2f():
    rng = np.random.default_rng(8)
    scores = np.concatenate([rng.uniform(0, 1, 4000), rng.uniform(0, 9.99, 1000)]).astype(np.float32)
    scores = np.concatenate([scores, np.float32([0.125, 0.375, 0.625, 0.875, 0.0, 0.005, 0.995, 1.0, 9.99])])
    for s in scores:
        assert vz.label_text(b'n', s) == ('n|%.2f' % float(s)).encode('ascii'), s
    assert vz.label_text(b'', np.float32(12.0)) == b'|9.99' and vz.label_text(b'', np.float32(-1.0)) == b'|0.00'


def test_label_sits_above_the_box_or_moves_inside():
    H, W = 40, 80
    for y0, top in ((9, 0), (20, 11), (8, 8), (0, 0)):
        rows = dc.empty_rows(1, 1)
        dc.set_row(rows, 0, (5, y0, 70, 39), 0.5, 0)
        got = vz.draw_restatement(_plain(H, W), rows, 1, ['ab'], thickness=1)
        lx0, ly0, lx1, ly1 = _label_rect(5, y0, 'ab')
        assert ly0 == top
        colour = vz.palette(1)[0]
        box = got[ly0:ly1 + 1, lx0:lx1 + 1]
        ink = (box != colour).any(axis=2)
        assert ink.any() and not ink[0].any() and not ink[-1].any() and not ink[:, 0].any() and not ink[:, -1].any()
        assert (got[ly1 + 1, lx1 + 1:W - 11] == (colour if ly1 + 1 == y0 else GREY)).all()


def test_glyphs_scale_and_an_unknown_byte_is_a_block():
    rows = dc.empty_rows(1, 1)
    dc.set_row(rows, 0, (2, 30, 50, 39), 0.5, 0)
    colour = vz.palette(1)[0]
    for s in (1, 2, 3):
        got = vz.draw_restatement(_plain(40, 120), rows, 1, ['~T'], font_scale=s)
        ink = (got[30 - 9 * s:30, 2:2 + 13 * s] != colour).any(axis=2)
        cell = ink.reshape(9, s, 13, s)
        assert (cell.all(axis=(1, 3)) == cell.any(axis=(1, 3))).all()          # s x s blocks
        small = cell.all(axis=(1, 3))
        assert small[1:8, 1:6].all() and not small[:, 0].any() and not small[:, 6].any() and not small[0].any() and not small[8].any()
        want_t = np.array([[(m >> (4 - c)) & 1 for c in range(5)] for m in vz.glyph_table()[ord('T')]], dtype=bool)
        assert np.array_equal(small[1:8, 7:12], want_t)
    table = vz.glyph_table()
    for ch in ' 0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ._|-':
        assert ch in vz.GLYPHS and (table[ord(ch)] <= 0x1F).all()
    drawn = [ch for ch in vz.GLYPHS if ch != ' ']
    assert len(set(table[ord(ch)].tobytes() for ch in drawn)) == len(drawn)      # no two glyphs alike
    assert (table[ord('~')] == vz.BLOCK).all() and (table[0xC3] == vz.BLOCK).all()


def test_palette_is_distinct_saturated_and_never_the_landmark_colour():
    for L in (1, 2, 3, 13, 14, 64):
        p = vz.palette(L)
        assert p.shape == (L, 3) and len(set(map(tuple, p.tolist()))) == L
        assert (p.max(axis=1) == 255).all() and (p.min(axis=1) == 0).all()
        assert tuple(vz.KPT_COLOR) not in set(map(tuple, p.tolist()))


def test_nothing_above_the_threshold_returns_the_source():
    img = dc.image(33, 65, seed=1)
    rows = dc.random_rows(2, 20, 3, 33, 65, 3)
    rows[:, 4] = np.minimum(rows[:, 4], np.float32(0.3))
    out = vz.draw_restatement(img, rows, 20, dc.NAMES3, contour=True)
    assert np.array_equal(out, img) and out is not img
    rows[:, 4] = 0.9
    assert np.array_equal(vz.draw_restatement(img, rows, 0, dc.NAMES3), img)
    assert (vz.draw_restatement(img, rows, 20, dc.NAMES3) != img).any()


def test_settings_outside_their_ranges_are_refused():
    img, rows = dc.image(8, 8), dc.empty_rows(1, 1)
    for kw in (dict(thickness=0), dict(thickness=65), dict(radius=0), dict(radius=65), dict(line_width=0), dict(line_width=17),
               dict(font_scale=0), dict(font_scale=9), dict(font_scale=1.5)):
        with pytest.raises(ValueError):
            vz.draw_restatement(img, rows, 1, ['a'], **kw)
    with pytest.raises(ValueError):
        vz.draw_restatement(img, rows, 1, ['a'] * 65)
    with pytest.raises(ValueError):
        vz.draw_restatement(img, rows, 1, ['x' * 256])
    with pytest.raises(TypeError):
        vz.draw_restatement(img.astype(np.float32), rows, 1, ['a'])


def test_show_result_on_the_cpu_draws_the_golden_demo_detections(tmp_path, monkeypatch):
    from PIL import Image
    from kgdet_amd import apis
    monkeypatch.setattr(vz, 'device_available', lambda: False)
    data = demo_cases.demo_dataset(test_mode=True)
    G = np.load(demo_checks.GOLDEN)
    result = demo_checks.golden_as_results(G, data, [0])[0]
    img = data.load_image(0)
    thr = float(np.sort(G['img0:bboxes'][:, 4])[len(G['img0:labels']) // 2])         # half of them above it
    drawn = apis.show_result(img, result, data.CLASSES, score_thr=thr, contour=True)
    assert drawn.shape == img.shape and drawn.dtype == np.uint8 and (drawn != img).any()
    rows, n = vz.result_rows(result)
    assert n == len(G['img0:labels']) and rows.shape == (n, 7 + 882)
    order = np.argsort(G['img0:labels'], kind='stable')
    assert np.array_equal(rows[:, :5], G['img0:bboxes'][order]) and np.array_equal(rows[:, 5], G['img0:labels'][order])
    ranges = vz.default_ranges(13, 294)
    assert np.array_equal(drawn, vz.draw_restatement(img, rows, n, data.CLASSES, landmark_ranges=ranges, score_thr=thr, contour=True))
    reds = (drawn == vz.KPT_COLOR).all(axis=2).sum()
    assert reds > 0 and (apis.show_result(img, result, data.CLASSES, score_thr=thr, kpt_color=None) == vz.KPT_COLOR).all(axis=2).sum() < reds
    path = str(tmp_path / 'shown.png')
    assert apis.show_result(img, result, data.CLASSES, score_thr=thr, contour=True, out_file=path) is None
    with Image.open(path) as im:
        assert np.array_equal(np.array(im.convert('RGB')), drawn)
    assert np.array_equal(apis.show_result(path, ([np.zeros((0, 5), np.float32)] * 13, ), data.CLASSES), drawn)   # nothing to draw
    with pytest.raises(NotImplementedError):
        apis.show_result(img, result, data.CLASSES, show=True)
