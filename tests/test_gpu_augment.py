"""``extra_aug`` on the GPU: the kernel ``kgdet_image_preprocess_aug`` (csrc/preprocess_aug.hip) through the C ABI, bit-equal to
``preprocess.image_transform_restatement_aug`` -- outputs pre-filled with NaN inside NaN canaries -- at the sizes where it can go
wrong (a palette of colour edge cases, tiny windows that straddle raw image and fill, destinations off the 16-byte grid, more
rows than the grid holds), its limits, and the training route ``datasets.collate_device`` with plans."""
import ctypes

import numpy as np
import pytest
import torch

from kgdet_amd import _lib, augment, datasets, preprocess, runner
from tests.golden import demo_cases

pytestmark = pytest.mark.gpu

NORM = demo_cases.IMG_NORM
MEAN, STD = NORM['mean'], NORM['std']


def _plan(h, w, **kw):
    p = augment.AugPlan(h, w, 0)
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _synthetic(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _palette():
    """12 x 18: every (r, g, b) of {0, 1, 127, 128, 254, 255}^3 -- grey, black, two equal maxima, each hue sector"""
    lv = np.array([0, 1, 127, 128, 254, 255], dtype=np.uint8)
    r, g, b = np.meshgrid(lv, lv, lv, indexing='ij')
    return np.ascontiguousarray(np.stack([r, g, b], axis=-1).reshape(12, 18, 3))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(cases, mean=MEAN, std=STD, to_rgb=True, size_divisor=None):
    """``cases``: dicts of raw (uint8 numpy, or a cuda view with its own pitch), plan, scale, flip, keep_ratio, out_hw, col0,
    extra_w.  ONE launch per KGDET_PREPROC_AUG_MAX_JOBS jobs through the C ABI; every destination is a [3, H, W] view one
    row and ``col0`` (>= 1) columns inside a NaN buffer.  Asserts bit equality with the restatement and untouched canaries."""
    T = preprocess.DeviceImageTransform(mean, std, to_rgb, size_divisor)
    L = _lib.lib()
    fp = ctypes.POINTER(ctypes.c_float)
    wants, bufs, views, srcs, size_plans = [], [], [], [], []
    for c in cases:
        raw = c['raw']
        host = raw.cpu().numpy() if isinstance(raw, torch.Tensor) else raw
        want, img_shape, pad_shape, _ = preprocess.image_transform_restatement_aug(
            np.ascontiguousarray(host), c.get('plan'), c['scale'], c.get('flip', False), c.get('keep_ratio', False), mean, std,
            to_rgb, size_divisor, c.get('out_hw'))
        H, W = want.shape[1:]
        col0 = c.get('col0', 4)
        buf = torch.full((3, H + 2, col0 + W + c.get('extra_w', 4)), float('nan'), device='cuda')
        wants.append(want)
        bufs.append(buf)
        views.append(buf[:, 1:H + 1, col0:col0 + W])
        srcs.append(raw if isinstance(raw, torch.Tensor) else torch.from_numpy(host).cuda())
        vh, vw = host.shape[:2] if c.get('plan') is None else c['plan'].virtual_hw
        size_plans.append(preprocess.plan(vh, vw, c['scale'], c.get('keep_ratio', False), size_divisor))
        assert size_plans[-1][2] == img_shape
    tables = T.aug_job_tables(srcs, size_plans, [c.get('flip', False) for c in cases], views, [c.get('plan') for c in cases])
    assert len(tables) == -(-len(cases) // _lib.PREPROC_AUG_MAX_JOBS)
    m32, s32 = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    for jobs in tables:
        rc = L.kgdet_image_preprocess_aug(jobs, ctypes.c_int32(len(jobs)), m32.ctypes.data_as(fp), s32.ctypes.data_as(fp),
                                          ctypes.c_int32(0 if to_rgb else 1), _lib.current_stream())
        assert rc == _lib.KGDET_OK, L.kgdet_last_error()
    torch.cuda.synchronize()
    for k, (c, want, buf, view) in enumerate(zip(cases, wants, bufs, views)):
        got = view.cpu()
        w = torch.from_numpy(want)
        assert not torch.isnan(got).any(), (k, c.get('name'))
        diff = _bits(got) != _bits(w)
        assert not diff.any(), (k, c.get('name'), int(diff.sum()), float((got - w).abs().max()))
        mask = torch.ones(buf.shape, dtype=torch.bool)
        col0 = c.get('col0', 4)
        mask[:, 1:1 + want.shape[1], col0:col0 + want.shape[2]] = False
        assert torch.isnan(buf.cpu()[mask]).all(), (k, c.get('name'), 'canary')
    return wants


# ---- colour ------------------------------------------------------------------------------------
ALL_ON = dict(colour=True, delta=-17.25, alpha=1.37, sat=0.81, hue=11.5, perm=(1, 2, 0))
COLOUR_PLANS = {
    'absent': dict(),
    'round_trip_only': dict(colour=True),
    'brightness': dict(colour=True, delta=20.5),
    'brightness_negative_values': dict(colour=True, delta=-300.0),
    'contrast_first': dict(colour=True, alpha=1.3, contrast_first=True),
    'contrast_last': dict(colour=True, alpha=0.6, contrast_first=False),
    'saturation': dict(colour=True, sat=0.7),
    'saturation_1.5': dict(colour=True, sat=1.5),
    'hue': dict(colour=True, hue=10.0),
    'hue_wraps_past_360': dict(colour=True, hue=350.0),
    'hue_wraps_below_0': dict(colour=True, hue=-350.0),
    'hue_limit': dict(colour=True, hue=-720.0, sat=1.5),
    'all_contrast_first': dict(ALL_ON, contrast_first=True),
    'all_contrast_last': dict(ALL_ON, contrast_first=False),
}
for _p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
    COLOUR_PLANS['perm_%d%d%d' % _p] = dict(colour=True, perm=_p, delta=3.0)


@pytest.mark.parametrize('name', sorted(COLOUR_PLANS))
def test_colour_stages_on_the_palette(name):
    """the identity resize shows every distorted palette pixel itself; the flipped 2.6x upscale interpolates between them"""
    raw = _palette()
    plan = _plan(12, 18, **COLOUR_PLANS[name])
    wants = _run([dict(raw=raw, plan=plan, scale=(18, 12), name=name),
                  dict(raw=raw, plan=plan, scale=(47, 31), flip=True, name=name + ' upscaled')])
    if name == 'absent':      # no colour stage at all: the pixels themselves
        assert np.array_equal(wants[0], ((raw.astype(np.float32) - np.float32(MEAN)) / np.float32(STD)).transpose(2, 0, 1))
    if name == 'brightness_negative_values':      # every value entering the HSV stage is negative
        assert int(raw.max()) + COLOUR_PLANS[name]['delta'] < 0


def test_the_six_permutations_differ_and_map_bgr_draws_to_rgb():
    assert augment.rgb_permutation((0, 1, 2)) == (0, 1, 2) and augment.rgb_permutation((1, 2, 0)) == (2, 0, 1)
    assert len({augment.rgb_permutation(p) for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))}) == 6


# ---- window ------------------------------------------------------------------------------------
WINDOWS = {
    'expand': lambda h, w: dict(canvas=(20, 30), top=3, left=5),
    'crop': lambda h, w: dict(patch=(2, 1, w - 1, h - 1)),
    'expand_and_crop_around_the_image': lambda h, w: dict(canvas=(20, 30), top=3, left=5, patch=(1, 2, 27, 19)),
    'crop_border_cuts_the_image': lambda h, w: dict(canvas=(20, 30), top=3, left=5, patch=(8, 5, 28, 18)),
    'crop_one_pixel': lambda h, w: dict(canvas=(20, 30), top=3, left=5, patch=(5, 3, 6, 4)),
}
SCALES = {'up': dict(scale=(64, 48), keep_ratio=True), 'down': dict(scale=(6, 5), keep_ratio=True),
          'up_free': dict(scale=(53, 41), keep_ratio=False), 'down_free': dict(scale=(5, 7), keep_ratio=False)}


@pytest.mark.parametrize('to_rgb', [True, False])
@pytest.mark.parametrize('window', sorted(WINDOWS))
def test_windows_on_tiny_images(window, to_rgb):
    """7 x 9 and 13 x 17 raw images; every scale rule, plain and flipped, with and without a colour stage, one launch each"""
    cases = []
    for h, w in ((7, 9), (13, 17)):
        raw = _synthetic(h, w, 100 * h + w)
        for colour in (dict(), ALL_ON):
            plan = _plan(h, w, fill=np.array([9.5, 130.25, 250.0], dtype=np.float32), **WINDOWS[window](h, w), **colour)
            for sname, s in sorted(SCALES.items()):
                for flip in (False, True):
                    cases.append(dict(raw=raw, plan=plan, flip=flip, name=(window, h, w, bool(colour), sname, flip), **s))
    _run(cases, to_rgb=to_rgb, size_divisor=None if to_rgb else 8)


def test_window_without_an_expand_fill_uses_the_mean_in_raw_order():
    raw = _synthetic(7, 9, 5)
    plan = _plan(7, 9, canvas=(20, 30), top=3, left=5)
    assert plan.fill is None
    for to_rgb in (True, False):
        want = _run([dict(raw=raw, plan=plan, scale=(30, 20))], to_rgb=to_rgb)[0]
        assert not want[:, :3].any() and not want[:, :, :5].any() and want[:, 3:10, 5:14].all()      # the mean normalises to 0


def _abi_job(src_t, dst_t, **kw):
    src, dst = src_t, dst_t
    f = dict(src=src.data_ptr(), src_h=src.shape[0], src_w=src.shape[1], src_row_bytes=src.stride(0), dst=dst.data_ptr(),
             dst_channel_stride=dst.stride(0), dst_row_stride=dst.stride(1), new_h=dst.shape[1], new_w=dst.shape[2],
             out_h=dst.shape[1], out_w=dst.shape[2], flip=0, vh=src.shape[0], vw=src.shape[1], oy=0, ox=0,
             fill=(ctypes.c_float * 3)(0, 0, 0), delta=0.0, alpha=0.0, sat=0.0, hue=0.0, perm=0 | 1 << 2 | 2 << 4, flags=0)
    f.update(kw)
    f.setdefault('scale_y', float(preprocess.axis_scale(f['vh'], f['new_h'])))
    f.setdefault('scale_x', float(preprocess.axis_scale(f['vw'], f['new_w'])))
    return _lib.PreprocAugJob(**f)


def _abi_call(jobs, n, mean=MEAN, std=STD, reverse=0):
    fp = ctypes.POINTER(ctypes.c_float)
    m32, s32 = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    arr = (_lib.PreprocAugJob * max(len(jobs), 1))(*jobs)
    return _lib.lib().kgdet_image_preprocess_aug(arr, ctypes.c_int32(n), m32.ctypes.data_as(fp), s32.ctypes.data_as(fp),
                                                 ctypes.c_int32(reverse), _lib.current_stream())


@pytest.mark.parametrize('oy,ox', [(100, 100), (-100, 3), (2, -50)])
def test_window_wholly_in_the_fill(oy, ox):
    """no tap reaches the raw image (all-0xFF, so any read would show).  The interpolation of a constant m is
    ``l0 * m + l1 * m``: exact -- the output is ONE value per channel, and 0 when m is the mean -- where the products are exact,
    which holds for the identity resize (weights 1 and 0, any m) and for the 2x upscale (weights 1/4 and 3/4, and 1 and 0 at
    the clamped border) of an m with at most 22 significant bits."""
    src = torch.full((7, 9, 3), 255, dtype=torch.uint8, device='cuda')
    short = [100.0, 116.5, 103.25]
    for new_hw, mean, fill in (((8, 10), MEAN, MEAN), ((8, 10), MEAN, [1.5, 2.5, 3.5]), ((16, 20), short, short),
                               ((16, 20), MEAN, [1.5, 2.5, 3.5])):
        for reverse in (0, 1):
            dst = torch.full((3,) + new_hw, float('nan'), device='cuda')
            raw_order = fill if not reverse else fill[::-1]           # fill[] is in the raw image's order
            job = _abi_job(src, dst, vh=8, vw=10, oy=oy, ox=ox, fill=(ctypes.c_float * 3)(*raw_order),
                           flags=_lib.AUG_COLOUR | _lib.AUG_HUE, hue=20.0)
            assert _abi_call([job], 1, mean=mean, reverse=reverse) == _lib.KGDET_OK, _lib.lib().kgdet_last_error()
            torch.cuda.synchronize()
            want = (np.float32(fill) - np.float32(mean)) / np.float32(STD)
            got = dst.cpu().numpy()
            for c in range(3):
                assert (got[c].view(np.uint32) == want[c:c + 1].view(np.uint32)).all(), (new_hw, fill, reverse, c)
            if fill is mean:
                assert not got.any()


# ---- layout ------------------------------------------------------------------------------------
@pytest.mark.parametrize('col0,extra_w', [(1, 2), (2, 1), (3, 3), (4, 1)])
def test_destinations_off_the_16_byte_grid_and_out_larger_than_new(col0, extra_w):
    """row starts 4 / 8 / 12 bytes off a 16-byte boundary, odd row and plane strides (the all-dword path), a slot larger than
    the resized image (zeros), nothing written outside the view"""
    raw = _synthetic(13, 17, col0)
    plan = _plan(13, 17, canvas=(20, 30), top=3, left=5, patch=(8, 5, 28, 18), **ALL_ON)
    _run([dict(raw=raw, plan=plan, scale=(53, 41), out_hw=(45, 61), col0=col0, extra_w=extra_w, flip=True),
          dict(raw=raw, plan=None, scale=(37, 22), out_hw=(24, 40), col0=col0, extra_w=extra_w + 1)])


def test_padded_source_pitch():
    big = torch.from_numpy(_synthetic(20, 31, 3)).cuda()
    raw = big[2:15, 5:22]                                         # 13 x 17, row pitch 93 bytes, 15 bytes into the row
    assert raw.stride(0) == 93 and not raw.is_contiguous()
    _run([dict(raw=raw, plan=_plan(13, 17, patch=(3, 2, 15, 12), **ALL_ON), scale=(64, 48), keep_ratio=True),
          dict(raw=raw, plan=None, scale=(64, 48), keep_ratio=True, flip=True)])


def test_more_rows_than_the_grid_cap_and_two_plans_in_one_launch():
    """two 1100 x 8 slots: 2200 rows over a grid of 2048, so the stride loop makes a second trip and changes job in it"""
    raw = _synthetic(13, 17, 8)
    _run([dict(raw=raw, plan=_plan(13, 17, canvas=(20, 30), top=3, left=5, **ALL_ON), scale=(8, 1100)),
          dict(raw=raw, plan=_plan(13, 17, patch=(3, 2, 15, 12), colour=True, sat=1.5, perm=(2, 1, 0)), scale=(8, 1100),
               flip=True)])


def _wide_cases():
    """2 x 5000 raw rows against the 1536-pixel staging buffer: the whole row and a 1537-wide patch take the per-tap fallback,
    1536- and 1400-wide patches (starting 100 pixels in) are staged, one of them next to a job without a colour stage"""
    raw = _synthetic(2, 5000, 21)
    return [dict(raw=raw, plan=_plan(2, 5000, **ALL_ON), scale=(1201, 3), name='whole row'),
            dict(raw=raw, plan=_plan(2, 5000, patch=(100, 0, 1637, 2), **ALL_ON), scale=(901, 3), flip=True, name='1537'),
            dict(raw=raw, plan=_plan(2, 5000, patch=(100, 0, 1636, 2), **ALL_ON), scale=(901, 3), name='1536'),
            dict(raw=raw, plan=_plan(2, 5000, patch=(100, 0, 1636, 2)), scale=(901, 3), name='no colour'),
            dict(raw=raw, plan=_plan(2, 5000, canvas=(4, 5200), top=1, left=150, patch=(100, 0, 1500, 3), **ALL_ON),
                 scale=(1777, 5), flip=True, name='1400 with fill')]


def test_rows_wider_than_the_staging_buffer_take_the_per_tap_path():
    _run(_wide_cases())


def test_per_tap_and_staged_variants_give_the_same_bits(monkeypatch):
    """KGDET_PREPROC_AUG_STAGE=0 (the measurement switch) sends every job per tap: the restatement's bits again"""
    monkeypatch.setenv('KGDET_PREPROC_AUG_STAGE', '0')
    raw = _synthetic(13, 17, 4)
    plan = _plan(13, 17, canvas=(20, 30), top=3, left=5, patch=(8, 5, 28, 18), **ALL_ON)
    _run(_wide_cases() + [dict(raw=_palette(), plan=_plan(12, 18, **ALL_ON), scale=(47, 31), flip=True),
                          dict(raw=raw, plan=plan, scale=(53, 41)), dict(raw=raw, plan=plan, scale=(5, 7), flip=True)])


def test_one_more_job_than_a_launch_holds_is_split_by_the_caller():
    n = _lib.PREPROC_AUG_MAX_JOBS + 1
    T = preprocess.DeviceImageTransform(MEAN, STD, True, 32)
    raws = [_synthetic(7 + k % 3, 9 + k % 4, k) for k in range(n)]
    plans = [None if k % 5 == 4 else _plan(r.shape[0], r.shape[1], canvas=(20, 30), top=k % 4, left=k % 7,
                                           **(ALL_ON if k % 2 else {})) for k, r in enumerate(raws)]
    scales, flips = [(40 + 8 * (k % 3), 32) for k in range(n)], [bool(k % 2) for k in range(n)]
    outs, metas = T.separate(raws, scales, flips, aug_plans=plans)
    img, metas2 = T(raws, scales, flips, common_size=True, aug_plans=plans)
    torch.cuda.synchronize()
    for k in range(n):
        want, img_shape, pad_shape, sf = preprocess.image_transform_restatement_aug(raws[k], plans[k], scales[k], flips[k], True,
                                                                                    MEAN, STD, True, 32)
        assert metas[k] == (img_shape, pad_shape, sf) == metas2[k]
        assert torch.equal(_bits(outs[k][0].cpu()), _bits(torch.from_numpy(want))), k
        same = preprocess.image_transform_restatement_aug(raws[k], plans[k], scales[k], flips[k], True, MEAN, STD, True, 32,
                                                          out_hw=tuple(img.shape[2:]))[0]
        assert torch.equal(_bits(img[k].cpu()), _bits(torch.from_numpy(same))), k


def test_all_none_plans_make_the_plain_launch():
    """an aug_plans list of None is the call without one: the quantised, table-normalised image of the plain kernel"""
    T = preprocess.DeviceImageTransform(MEAN, STD, True, 32)
    raws = [_synthetic(40, 52, 1), _synthetic(33, 47, 2)]
    a, ma = T.separate(raws, [(96, 64)] * 2, [False, True], aug_plans=[None, None])
    b, mb = T.separate(raws, [(96, 64)] * 2, [False, True])
    assert ma == mb and all(torch.equal(x, y) for x, y in zip(a, b))
    want = preprocess.image_transform_restatement(raws[0], (96, 64), False, True, MEAN, STD, True, 32)[0]
    assert torch.equal(a[0][0].cpu(), torch.from_numpy(want))
    with pytest.raises(ValueError):
        T.separate(raws, [(96, 64)] * 2, [False, True], aug_plans=[None])
    with pytest.raises(ValueError):
        T.separate(raws, [(96, 64)] * 2, [False, True], aug_plans=[None, _plan(7, 9, colour=True)])


# ---- C ABI limits ------------------------------------------------------------------------------
def test_c_abi_limits_are_reported():
    L = _lib.lib()
    src = torch.from_numpy(_synthetic(16, 24, 0)).cuda()
    dst = torch.full((3, 8, 12), float('nan'), device='cuda')
    assert _abi_call([], 0) == _lib.KGDET_OK
    assert L.kgdet_image_preprocess_aug(None, ctypes.c_int32(0), None, None, ctypes.c_int32(0), None) == _lib.KGDET_OK
    assert L.kgdet_image_preprocess_aug((_lib.PreprocAugJob * 1)(_abi_job(src, dst)), ctypes.c_int32(1), None, None,
                                        ctypes.c_int32(0), None) == _lib.KGDET_E_SHAPE               # null mean / std
    assert b'null pointer' in L.kgdet_last_error()
    colour = _lib.AUG_COLOUR
    for bad in (dict(src=0), dict(dst=0), dict(vw=0, scale_x=1.0), dict(vh=-3, scale_y=1.0), dict(src_h=0), dict(new_w=0), dict(out_h=7),
                dict(src_row_bytes=71), dict(dst_row_stride=11), dict(dst_channel_stride=0), dict(scale_x=0.0),
                dict(scale_y=float('nan')), dict(ox=1 << 21), dict(oy=-(1 << 21)),
                dict(flags=colour | _lib.AUG_PERMUTE, perm=0), dict(flags=colour | _lib.AUG_PERMUTE, perm=3 | 1 << 2 | 2 << 4),
                dict(flags=colour | _lib.AUG_PERMUTE, perm=0 | 1 << 2 | 2 << 4 | 1 << 6), dict(flags=_lib.AUG_HUE),
                dict(flags=128), dict(flags=colour | _lib.AUG_HUE, hue=721.0),
                dict(flags=colour | _lib.AUG_BRIGHTNESS, delta=float('inf')),
                dict(flags=colour | _lib.AUG_CONTRAST, alpha=float('nan')), dict(flags=colour | _lib.AUG_SATURATION, sat=1e6)):
        assert _abi_call([_abi_job(src, dst, **bad)], 1) == _lib.KGDET_E_SHAPE, bad
        assert b'image_preprocess_aug' in L.kgdet_last_error(), bad
    assert _abi_call([_abi_job(src, dst)], -1) == _lib.KGDET_E_SHAPE
    many = [_abi_job(src, dst)] * (_lib.PREPROC_AUG_MAX_JOBS + 1)
    assert _abi_call(many, len(many)) == _lib.KGDET_E_UNSUPPORTED
    assert b'limit' in L.kgdet_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(dst).all()                                  # no rejected call wrote anything
    assert _abi_call([_abi_job(src, dst)], 1) == _lib.KGDET_OK
    torch.cuda.synchronize()
    want = preprocess.image_transform_restatement_aug(src.cpu().numpy(), None, (12, 8), False, False, MEAN, STD)[0]
    assert torch.equal(_bits(dst.cpu()), _bits(torch.from_numpy(want)))


# ---- the training route ------------------------------------------------------------------------
EXTRA_AUG = dict(photo_metric_distortion=dict(brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5),
                                              hue_delta=18),
                 expand=dict(mean=NORM['mean'], to_rgb=NORM['to_rgb'], ratio_range=(1, 2)),
                 random_crop=dict(min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.3))


def test_collate_device_with_plans_equals_collate_of_host_samples_and_trains():
    kw = dict(test_mode=False, flip_ratio=0.5, img_scale=[(640, 384), (512, 320)], extra_aug=EXTRA_AUG, with_crowd=True)
    data, ref = demo_cases.demo_dataset(**kw), demo_cases.demo_dataset(**kw)
    idx = [0, 3, 5, 6]
    np.random.seed(77)
    want = datasets.collate([ref.prepare_train_img(i) for i in idx])
    np.random.seed(77)
    samples = [data.prepare_train_raw(i) for i in idx]
    got = datasets.collate_device(samples, data.device_transform())
    plans = [s['aug_plan'] for s in samples]
    assert any(p.canvas is not None for p in plans) and any(p.patch is not None for p in plans)
    assert set(got) == set(want)
    assert got['img'].is_cuda and torch.equal(_bits(got['img'].cpu()), _bits(want['img']))
    for key in want:
        if key in ('img', 'img_meta'):
            continue
        assert all(torch.equal(g, w) for g, w in zip(got[key], want[key])), key
    for g, w in zip(got['img_meta'], want['img_meta']):
        assert all(g[k] == w[k] for k in ('img_shape', 'pad_shape', 'scale_factor', 'flip', 'ori_shape'))
    _, model = demo_cases.demo_detector()
    model = model.cuda().train()
    sub = slice(0, 2)
    losses = model(got['img'][sub], got['img_meta'][sub], return_loss=True,
                   gt_bboxes=[t.cuda() for t in got['gt_bboxes'][sub]], gt_labels=[t.cuda() for t in got['gt_labels'][sub]],
                   gt_keypoints=[t.cuda() for t in got['gt_keypoints'][sub]])
    loss, _ = runner.parse_losses(losses)
    assert torch.isfinite(loss)
