"""``extra_aug`` on the CPU: ``kgdet_amd.augment`` (draws, ground truth) and ``preprocess.image_transform_restatement_aug`` (pixels).

* the draws, the arithmetic order, the ``int()`` places and ``RandomCrop``'s quirks against the REFERENCE's own ``extra_aug.py``
  run in place with the identity for ``mmcv.bgr2hsv`` / ``hsv2bgr`` (tests/golden/make_extra_aug_golden.py) -- bit for bit;
* the two colour conversions, which are this project's definition (no mmcv / cv2 here), against a ``colorsys`` formulation in
  float64, and the float32 restatement against its own float64 evaluation within a bound counted from the expression;
* the window against a second formulation that materialises the canvas; ``apply_gt``; the dataset routes."""
import colorsys
import os

import numpy as np
import pytest
import torch

from kgdet_amd import augment, datasets, preprocess
from tests.golden import demo_cases, make_extra_aug_golden as golden

U = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'extra_aug_golden.npz')
# the reference's image is BGR: with the identity conversions its "h" is B, its "s" is G and its "v" is R
IDENTITY = (lambda r, g, b: (b, g, r), lambda h, s, v: (v, s, h))
CASES = [(name, seed) for name in sorted(golden.CONFIGS) for seed in golden.SEEDS]


def _plan(h, w, n=0, **kw):
    p = augment.AugPlan(h, w, n)
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _virtual_image(rgb_u8, plan, conversions=None):
    """the float32 RGB image the resize reads, through the restatement itself: at the virtual image's own size every tap has
    weight 1 or 0 (src = d exactly), and mean 0 / std 1 normalise nothing"""
    vh, vw = plan.virtual_hw
    out, img_shape, _, _ = preprocess.image_transform_restatement_aug(rgb_u8, plan, (vw, vh), False, False,
                                                                      conversions=conversions)
    assert img_shape == (vh, vw, 3)
    return out.transpose(1, 2, 0)


# ---- against the reference ---------------------------------------------------------------------
@pytest.fixture(scope='module')
def recorded():
    return np.load(GOLDEN)


@pytest.mark.parametrize('name,seed', CASES)
def test_draws_boxes_and_pixels_equal_the_reference(recorded, name, seed):
    key = '%s_%d_' % (name, seed)
    img, boxes, labels = recorded[key + 'img'], recorded[key + 'boxes'], recorded[key + 'labels']
    boxes_before, labels_before = boxes.copy(), labels.copy()
    np.random.seed(seed)
    plan = augment.ExtraAugmentation(**golden.CONFIGS[name]).draw(img.shape[0], img.shape[1], boxes, labels)
    assert np.random.randint(1 << 30) == int(recorded[key + 'next_draw'])           # the same number of draws
    got_boxes, got_labels, _, _ = plan.apply_gt(boxes, labels)
    assert np.array_equal(boxes, boxes_before) and np.array_equal(labels, labels_before)      # inputs not modified
    want = recorded[key + 'out_boxes']
    assert got_boxes.dtype == want.dtype == np.float32 and got_boxes.shape == want.shape
    assert np.array_equal(got_boxes.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got_labels, recorded[key + 'out_labels'])
    got = _virtual_image(np.ascontiguousarray(img[..., ::-1]), plan, IDENTITY)[..., ::-1]       # RGB in, BGR compared
    want = recorded[key + 'out_img']
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), want.view(np.uint32))


def test_the_recorded_cases_cover_each_transform_and_each_draw(recorded):
    seen = dict(expand=0, crop=0, both=0, delta=0, first=0, last=0, sat=0, hue=0, perm=set(), dropped=0)
    for name, seed in CASES:
        key = '%s_%d_' % (name, seed)
        np.random.seed(seed)
        img = recorded[key + 'img']
        p = augment.ExtraAugmentation(**golden.CONFIGS[name]).draw(img.shape[0], img.shape[1], recorded[key + 'boxes'],
                                                                   recorded[key + 'labels'])
        seen['expand'] += p.canvas is not None
        seen['crop'] += p.patch is not None
        seen['both'] += p.canvas is not None and p.patch is not None
        seen['delta'] += p.delta is not None
        seen['first'] += p.alpha is not None and p.contrast_first
        seen['last'] += p.alpha is not None and not p.contrast_first
        seen['sat'] += p.sat is not None
        seen['hue'] += p.hue is not None
        seen['dropped'] += int((~p.keep).sum())
        if p.perm is not None:
            seen['perm'].add(p.perm)
        assert p.colour == (name in ('photo', 'all'))
    assert all(seen[k] > 0 for k in ('expand', 'crop', 'both', 'delta', 'first', 'last', 'sat', 'hue')), seen
    assert len(seen['perm']) >= 4, seen


def test_bbox_overlaps_restated_keeps_float32_and_the_plus_one_extents():
    a = np.array([[0, 0, 9, 9]], dtype=np.int64)
    b = np.array([[0, 0, 9, 9], [5, 5, 14, 14], [10, 10, 12, 12]], dtype=np.float32)
    got = augment.bbox_overlaps(a, b)
    assert got.dtype == np.float32 and got.shape == (1, 3)
    assert got[0, 0] == 1 and got[0, 1] == np.float32(25) / np.float32(175) and got[0, 2] == 0
    assert np.array_equal(augment.bbox_overlaps(b, a), got.T)                      # (the exchange branch)
    assert augment.bbox_overlaps(a, b[:0]).shape == (1, 0)


def test_rgb_permutation_of_a_bgr_draw():
    bgr = np.arange(6, dtype=np.float32).reshape(2, 3)
    for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        q = augment.rgb_permutation(p)
        assert np.array_equal(bgr[:, ::-1][:, list(q)], bgr[:, list(p)][:, ::-1])       # the same picture


# ---- the conversions ---------------------------------------------------------------------------
def _pixels():
    """20 000 random uint8 pixels + every grey + pixels with two equal channels (uint8: diff is 0 or >= 1)"""
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, (20000, 3))
    grey = np.repeat(np.arange(256)[:, None], 3, axis=1)
    two = rng.integers(0, 256, (3000, 3))
    two[:1000, 1] = two[:1000, 0]
    two[1000:2000, 2] = two[1000:2000, 1]
    two[2000:, 0] = two[2000:, 2]
    return np.concatenate([px, grey, two]).astype(np.float64)


def _settings():
    rng = np.random.default_rng(6)
    return [(None, None), (1.5, 18.0), (0.5, -18.0)] + [(float(rng.uniform(0.5, 1.5)), float(rng.uniform(-18, 18)))
                                                        for _ in range(5)]


def test_conversions_in_float64_agree_with_colorsys():
    """|difference| <= 1e-4 grey levels.  The two EPS = 2^-23 terms are all that separates the formulas: they move h by at most
    60 * 2^-23 degrees and s by 2^-23 relative, i.e. a channel by at most 255 * 1.5 * 1.2e-7, twice -- below 1e-4."""
    px = _pixels()
    worst = 0.0
    for sat, hue in _settings():
        plan = _plan(1, len(px), colour=True, sat=sat, hue=hue)
        got = preprocess.distort_restatement(px[None], plan)[0]
        assert got.dtype == np.float64
        sat32, hue32 = (1.0 if sat is None else float(np.float32(sat))), (0.0 if hue is None else float(np.float32(hue)))
        want = np.empty_like(px)
        for i, (r, g, b) in enumerate(px / 255.0):
            h, s, v = colorsys.rgb_to_hsv(r, g, b)
            h = (h * 360.0 + hue32) % 360.0 / 360.0
            want[i] = colorsys.hsv_to_rgb(h, s * sat32, v)
        worst = max(worst, float(np.abs(got - want * 255.0).max()))
    print('float64 restatement against colorsys: %.3g grey levels' % worst)
    assert worst <= 1e-4


def test_float32_restatement_stays_within_the_counted_bound_of_its_float64_evaluation():
    """Stages 3-6 on uint8 pixels, saturation in [0.5, 1.5], hue in +-18.  With V = max(r, g, b), D = V - min and A = D * sat
    (= V * s), the output is continuous and piecewise linear in h with slope at most A / 60 per degree (across the sector
    borders and the 360 wrap too, so a border that falls differently in the two precisions costs nothing more), and v, vmin,
    D, g - b and f = h - floor(h) are exact.  First order, U = 2^-24 per rounding, each rounding at most U times the largest
    magnitude its result can have:
      h in degrees: (g - b) * d carries 2 roundings of d and its own, |.| <= 60 (180); + 120 / 240 (300); + 360 (360); + dh
      (378); the wrap (360); * float32(6 / 360), the constant's own rounding and the product's (378 + 378); the sector loop
      (360) -- 2694 U degrees, 44.9 U in f, at most 44.9 U A in a channel;
      s: V + EPS, the division, * sat (3 U, at most 3 U A through s * f); the products s * f and s * (1 - f) and the
      difference 1 - f (3 U A); 1 - s * f lies in [-0.5, 1] (U V) and the final product (U V).
    bound = 1.01 * U * (51 A + 2 V): at most 1.2e-3 grey levels, the 1.01 for the second-order terms."""
    px = _pixels()
    V, D = px.max(axis=1), px.max(axis=1) - px.min(axis=1)
    worst = 0.0
    for sat, hue in _settings():
        plan = _plan(1, len(px), colour=True, sat=sat, hue=hue)
        got = preprocess.distort_restatement(px[None].astype(np.float32), plan)[0]
        assert got.dtype == np.float32
        want = preprocess.distort_restatement(px[None], plan)[0]
        bound = 1.01 * U * (51 * D * (1.0 if sat is None else sat) + 2 * V)
        frac = np.abs(got.astype(np.float64) - want) / np.maximum(bound, 1e-300)[:, None]
        frac[np.abs(got.astype(np.float64) - want) == 0] = 0
        worst = max(worst, float(frac.max()))
    print('float32 restatement against float64: %.3f of the bound (bound <= %.3g grey levels)'
          % (worst, 1.01 * U * (51 * 382.5 + 510)))
    assert worst <= 1.0


def test_round_trip_runs_whenever_photometric_distortion_is_configured():
    px = _pixels()[None, :2000].astype(np.float32)
    plain = preprocess.distort_restatement(px, _plan(1, 2000))
    assert plain is px                                                      # no colour stage at all
    rt = preprocess.distort_restatement(px, _plan(1, 2000, colour=True))
    assert rt.dtype == np.float32 and not np.array_equal(rt, px) and np.abs(rt - px).max() < 1e-3
    grey = np.repeat(np.arange(256, dtype=np.float32)[None, :, None], 3, axis=2)
    assert np.array_equal(preprocess.distort_restatement(grey, _plan(1, 256, colour=True, sat=1.5, hue=-18.0)), grey)


# ---- the window --------------------------------------------------------------------------------
def _materialised(rgb_u8, plan, scale, flip, keep_ratio, mean, std, to_rgb, size_divisor):
    """the second formulation: build the canvas, paste the distorted image, slice the patch, then resize that array"""
    img = preprocess.distort_restatement(rgb_u8.astype(np.float32), plan)
    fill = preprocess.aug_fill(plan, mean, to_rgb)
    if plan.canvas is not None:
        canvas = np.empty(plan.canvas + (3,), dtype=np.float32)
        canvas[:] = fill
        canvas[plan.top:plan.top + plan.h, plan.left:plan.left + plan.w] = img
        img = canvas
    if plan.patch is not None:
        x1, y1, x2, y2 = plan.patch
        img = img[y1:y2, x1:x2]
    vh, vw = img.shape[:2]
    new_h, new_w, img_shape, pad_shape, sf = preprocess.plan(vh, vw, scale, keep_ratio, size_divisor)
    out = np.zeros((3,) + pad_shape[:2], dtype=np.float32)
    sy, sx = preprocess.axis_scale(vh, img_shape[0]), preprocess.axis_scale(vw, img_shape[1])
    m, s = np.float32(mean), np.float32(std)
    for y in range(img_shape[0]):
        src = max(np.float32(sy * np.float32(y + 0.5)) - np.float32(0.5), np.float32(0))
        y0 = min(int(src), vh - 1)
        y1_, ly1 = y0 + (y0 < vh - 1), src - np.float32(y0)
        for x in range(img_shape[1]):
            srx = max(np.float32(sx * np.float32(x + 0.5)) - np.float32(0.5), np.float32(0))
            x0 = min(int(srx), vw - 1)
            x1_, lx1 = x0 + (x0 < vw - 1), srx - np.float32(x0)
            lx0, ly0 = np.float32(1) - lx1, np.float32(1) - ly1
            v = ly0 * (lx0 * img[y0, x0] + lx1 * img[y0, x1_]) + ly1 * (lx0 * img[y1_, x0] + lx1 * img[y1_, x1_])
            if not to_rgb:
                v = v[::-1]
            out[:, y, img_shape[1] - 1 - x if flip else x] = (v - m) / s
    return out, img_shape, pad_shape, sf


WINDOWS = [dict(canvas=(20, 30), top=3, left=5), dict(patch=(2, 1, 8, 6)), dict(canvas=(20, 30), top=3, left=5, patch=(1, 2, 27, 19)),
           dict(canvas=(20, 30), top=3, left=5, patch=(8, 5, 13, 9)), dict(canvas=(20, 30), top=0, left=21, patch=(5, 3, 6, 4)),
           dict()]


@pytest.mark.parametrize('window', range(len(WINDOWS)))
def test_window_equals_the_materialised_canvas(window):
    raw = np.random.default_rng(window).integers(0, 256, (7, 9, 3), dtype=np.uint8)
    colour = dict(colour=True, delta=-17.25, alpha=1.37, sat=0.81, hue=11.5, perm=(1, 2, 0))
    for k, (scale, keep_ratio, flip, to_rgb, div) in enumerate([((40, 30), True, False, True, None), ((6, 5), True, True, False, 8),
                                                                ((23, 17), False, True, True, 4), ((4, 9), False, False, False, None)]):
        fill = None if k == 0 else np.array([9.5, 130.25, 250.0], dtype=np.float32)
        plan = _plan(7, 9, fill=fill, **WINDOWS[window], **(colour if k % 2 else {}))
        args = (scale, flip, keep_ratio, demo_cases.IMG_NORM['mean'], demo_cases.IMG_NORM['std'], to_rgb, div)
        got = preprocess.image_transform_restatement_aug(raw, plan, *args)
        want = _materialised(raw, plan, *args)
        assert got[1] == want[1] and got[2] == want[2] and np.array_equal(got[3], want[3])
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (window, k)


def test_no_plan_is_the_identity_window_and_out_hw_pads():
    raw = np.random.default_rng(0).integers(0, 256, (7, 9, 3), dtype=np.uint8)
    a = preprocess.image_transform_restatement_aug(raw, None, (40, 30), True, True, (1, 2, 3), (4, 5, 6), True, 32)
    b = preprocess.image_transform_restatement_aug(raw, _plan(7, 9), (40, 30), True, True, (1, 2, 3), (4, 5, 6), True, 32)
    assert np.array_equal(a[0], b[0]) and a[1:3] == b[1:3] and a[0].shape == (3, 32, 64)
    c = preprocess.image_transform_restatement_aug(raw, None, (40, 30), True, True, (1, 2, 3), (4, 5, 6), True, 32, out_hw=(40, 70))
    assert c[2] == a[2] and np.array_equal(c[0][:, :32, :64], a[0]) and not c[0][:, 32:].any() and not c[0][:, :, 64:].any()
    # unlike the plain route nothing is quantised: an upscale keeps fractional grey levels
    v = a[0][:, :a[1][0], :a[1][1]] * np.float32([4, 5, 6])[:, None, None] + np.float32([1, 2, 3])[:, None, None]
    assert np.abs(v - np.rint(v)).max() > 0.2


# ---- the ground truth --------------------------------------------------------------------------
def test_apply_gt_moves_landmarks_and_ignore_boxes_and_modifies_nothing():
    boxes = np.array([[2, 2, 10, 8], [20, 3, 28, 9], [12, 10, 16, 14]], dtype=np.float32)
    labels = np.array([3, 7, 9])
    kp = [np.zeros((294, 3)) for _ in range(3)]
    kp[0][5] = (4, 4, 2)          # inside the patch after the shift
    kp[0][6] = (1, 1, 1)          # labelled, falls left of / above the patch
    kp[0][7] = (0, 0, 0)          # unlabelled: stays (0, 0, 0), is not shifted
    kp[1][0] = (22, 5, 2)
    kp[2][1] = (13, 11, 1)
    kp[2][2] = (18, 14, 2)        # lands exactly on x = patch_w: outside [0, patch_w)
    ignore = np.array([[0, 0, 3, 3], [6, 6, 30, 12], [25, 0, 29, 2]], dtype=np.float32)
    before = [boxes.copy(), labels.copy(), [k.copy() for k in kp], ignore.copy()]
    plan = _plan(16, 30, 3, canvas=(40, 60), top=4, left=6, patch=(8, 5, 24, 20), keep=np.array([True, False, True]))
    assert plan.virtual_hw == (15, 16) and plan.origin == (-1, -2)
    b, l, k, ig = plan.apply_gt(boxes, labels, kp, ignore)
    for x, y in zip([boxes, labels, ignore], [before[0], before[1], before[3]]):
        assert np.array_equal(x, y)
    assert all(np.array_equal(x, y) for x, y in zip(kp, before[2]))
    # boxes: + (6, 4), mask, clip to the patch, - (8, 5)
    assert b.dtype == np.float32 and np.array_equal(b, [[0, 1, 8, 7], [10, 9, 14, 13]]) and np.array_equal(l, [3, 9])
    assert len(k) == 2 and k[0].shape == (294, 3)
    assert tuple(k[0][5]) == (2, 3, 2) and tuple(k[0][6]) == (0, 0, 0) and tuple(k[0][7]) == (0, 0, 0)
    assert tuple(k[1][1]) == (11, 10, 1) and tuple(k[1][2]) == (0, 0, 0)
    assert int((k[0][:, 2] != 0).sum()) == 1 and int((k[1][:, 2] != 0).sum()) == 1
    # ignore boxes, shifted: [6,4,9,7] overlaps the patch's corner and is clipped to it; [12,10,36,16] is clipped at x2 = 24;
    # [31,4,35,6] lies right of the patch and is dropped
    assert np.array_equal(ig, [[0, 0, 1, 2], [4, 5, 16, 11]])
    # a landmark on the last column / row of the patch stays
    kp2 = [np.zeros((294, 3))]
    kp2[0][0] = (17, 15, 2)
    last = _plan(16, 30, 1, canvas=(40, 60), top=4, left=6, patch=(8, 5, 24, 20)).apply_gt(boxes[:1], labels[:1], kp2)[2]
    assert tuple(last[0][0]) == (15, 14, 2)


def test_apply_gt_without_a_crop_only_shifts():
    boxes = np.array([[2, 2, 10, 8]], dtype=np.float32)
    kp = [np.zeros((294, 3))]
    kp[0][3] = (4.5, 6, 1)
    ignore = np.array([[0, 0, 3, 3]], dtype=np.float32)
    b, l, k, ig = _plan(16, 30, 1, canvas=(40, 60), top=4, left=6).apply_gt(boxes, np.array([2]), kp, ignore)
    assert np.array_equal(b, [[8, 6, 16, 12]]) and np.array_equal(ig, [[6, 4, 9, 7]]) and tuple(k[0][3]) == (10.5, 10, 1)
    b, l, k, ig = _plan(16, 30, 1, colour=True).apply_gt(boxes, np.array([2]), kp, None)
    assert np.array_equal(b, boxes) and b is not boxes and ig is None and np.array_equal(k[0], kp[0])


# ---- the dataset -------------------------------------------------------------------------------
EXTRA_AUG = dict(photo_metric_distortion=dict(brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5),
                                              hue_delta=18),
                 expand=dict(mean=demo_cases.IMG_NORM['mean'], to_rgb=demo_cases.IMG_NORM['to_rgb'], ratio_range=(1, 2)),
                 random_crop=dict(min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.3))
SMALL = dict(test_mode=False, flip_ratio=0.5, img_scale=[(320, 192), (256, 160)], with_crowd=True)


def test_dataset_with_extra_aug_host_route_equals_the_restatement_on_the_raw_sample():
    data = demo_cases.demo_dataset(extra_aug=EXTRA_AUG, **SMALL)
    norm = demo_cases.IMG_NORM
    np.random.seed(31)
    want = [data.prepare_train_img(i) for i in range(8)]
    state_after = np.random.get_state()[1].copy()
    np.random.seed(31)
    got = [data.prepare_train_raw(i) for i in range(8)]
    assert np.array_equal(np.random.get_state()[1], state_after)
    kinds = set()
    for idx, (g, w) in enumerate(zip(got, want)):
        assert g is not None and w is not None
        plan = g['aug_plan']
        kinds |= {('canvas', plan.canvas is not None), ('patch', plan.patch is not None)}
        info = data.img_infos[idx]
        assert (plan.h, plan.w) == (info['height'], info['width']) and plan.colour
        img, img_shape, pad_shape, sf = preprocess.image_transform_restatement_aug(
            g['raw'], plan, g['scale'], g['flip'], g['keep_ratio'], norm['mean'], norm['std'], norm['to_rgb'], 32)
        assert np.array_equal(img.view(np.uint32), w['img'].numpy().view(np.uint32))
        gm, wm = g['img_meta'], w['img_meta']
        for key in ('ori_shape', 'img_shape', 'pad_shape', 'scale_factor', 'flip'):
            assert gm[key] == wm[key], key
        assert gm['ori_shape'] == (info['height'], info['width'], 3)                  # the file's, not the virtual image's
        assert gm['img_shape'] == img_shape and gm['pad_shape'] == pad_shape and tuple(w['img'].shape) == (3,) + pad_shape[:2]
        vh, vw = plan.virtual_hw
        assert img_shape[0] == int(vh * sf + 0.5) and img_shape[1] == int(vw * sf + 0.5)
        assert set(g) - {'raw', 'scale', 'flip', 'keep_ratio', 'aug_plan'} == set(w) - {'img'}
        for key in ('gt_bboxes', 'gt_labels', 'gt_bboxes_ignore', 'gt_keypoints'):
            assert g[key].dtype == w[key].dtype and torch.equal(g[key], w[key]), key
        n = int(plan.keep.sum())
        assert len(g['gt_bboxes']) == len(g['gt_labels']) == len(g['gt_keypoints']) == n >= 1
        assert tuple(g['gt_keypoints'].shape[1:]) == (294, 3)
        b = g['gt_bboxes']
        assert (b[:, 0] >= 0).all() and (b[:, 2] <= img_shape[1] - 1).all() and (b[:, 3] <= img_shape[0] - 1).all()
        kp = g['gt_keypoints']
        on = kp[..., 2] != 0
        assert (kp[..., 0][on] >= 0).all() and (kp[..., 0][on] <= img_shape[1]).all() and (kp[..., 1][on] <= img_shape[0]).all()
    assert kinds >= {('canvas', True), ('canvas', False), ('patch', True)}, kinds        # (a crop is declined 1 time in 7)
    batch = datasets.collate(want[:3])
    assert batch['img'].shape[0] == 3 and len(batch['gt_keypoints']) == 3


def test_dataset_without_extra_aug_draws_and_returns_what_it_did():
    data = demo_cases.demo_dataset(**SMALL)
    assert data.extra_aug is None
    np.random.seed(9)
    got = data.prepare_train_img(2)
    state_after = np.random.get_state()[1].copy()
    np.random.seed(9)
    flip = bool(np.random.rand() < data.flip_ratio)                          # the two draws there have always been
    scale = data._sample_scale()
    assert np.array_equal(np.random.get_state()[1], state_after)
    img, img_shape, pad_shape, sf = data.img_transform(data.load_image(2), scale, flip, keep_ratio=True)
    assert np.array_equal(got['img'].numpy(), img) and got['img_meta']['img_shape'] == img_shape
    ann = data.get_ann_info(2)
    assert torch.equal(got['gt_bboxes'], torch.from_numpy(datasets.bbox_transform(ann['bboxes'], img_shape, sf, flip)))
    np.random.seed(9)
    assert 'aug_plan' not in data.prepare_train_raw(2)


def test_test_mode_ignores_extra_aug_and_the_other_keywords_still_raise():
    data = demo_cases.demo_dataset(test_mode=True, extra_aug=EXTRA_AUG)
    assert data.extra_aug is None
    plain = demo_cases.demo_dataset(test_mode=True)
    state = np.random.get_state()[1].copy()
    a, b = data.prepare_test_img(0), plain.prepare_test_img(0)
    assert np.array_equal(np.random.get_state()[1], state)
    assert torch.equal(a['img'][0], b['img'][0])
    for kw in (dict(with_mask=True), dict(proposal_file='p.pkl'), dict(corruption='fog'), dict(with_semantic_seg=True)):
        with pytest.raises(NotImplementedError):
            demo_cases.demo_dataset(test_mode=False, **kw)
