"""Device image preprocessing on the GPU: the kernel (csrc/preprocess.hip) bit-exact against the restatement
``preprocess.image_transform_restatement``, the demo set end to end through ``runner.single_gpu_test(device_preprocess=True)``,
the graphed inference route writing into ``run.static_img``, the training batch of ``datasets.collate_device`` and the C ABI's
limits."""
import ctypes

import numpy as np
import pytest
import torch

from kgdet_amd import _lib, datasets, preprocess, runner
from tests.golden import demo_cases

pytestmark = pytest.mark.gpu

NORM = demo_cases.IMG_NORM
SCALES = [(1333, 800), (1000, 600)]


def _transform(to_rgb=True, size_divisor=32, mean=None, std=None):
    return preprocess.DeviceImageTransform(NORM['mean'] if mean is None else mean, NORM['std'] if std is None else std, to_rgb,
                                           size_divisor)


def _restated(T, raw, scale, flip, keep_ratio=True, out_hw=None):
    raw = raw.cpu().numpy() if isinstance(raw, torch.Tensor) else raw
    return image_restated(T, raw, scale, flip, keep_ratio, out_hw)


def image_restated(T, raw, scale, flip, keep_ratio, out_hw):
    return preprocess.image_transform_restatement(raw, scale, flip, keep_ratio, T.mean, T.std, T.to_rgb, T.size_divisor, out_hw)


def _check_separate(T, raws, scales, flips, keep_ratio=True):
    outs, metas = T.separate(raws, scales, flips, keep_ratio=keep_ratio)
    torch.cuda.synchronize()
    assert len(outs) == len(metas) == len(raws)
    for o, m, r, s, f in zip(outs, metas, raws, scales, flips):
        want, img_shape, pad_shape, sf = _restated(T, r, s, f, keep_ratio)
        assert o.is_cuda and o.dtype == torch.float32 and tuple(o.shape) == (1,) + want.shape
        assert m[0] == img_shape and m[1] == pad_shape and np.array_equal(m[2], sf)
        got = o[0].cpu()
        assert torch.equal(got, torch.from_numpy(want)), (tuple(r.shape), s, f, int((got != torch.from_numpy(want)).sum()))


def _synthetic(h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


@pytest.fixture(scope='module')
def demo_images():
    data = demo_cases.demo_dataset(test_mode=True)
    return [torch.from_numpy(data.load_image(i)) for i in range(0, 32, 4)]


def test_kernel_matches_restatement_on_demo_images_one_source_four_jobs(demo_images):
    """every fourth demo image, both scales x flip from ONE uploaded copy"""
    T = _transform()
    assert len({tuple(r.shape) for r in demo_images}) > 2
    for raw in demo_images:
        _check_separate(T, [raw] * 4, [SCALES[0], SCALES[0], SCALES[1], SCALES[1]], [False, True, False, True])


@pytest.mark.parametrize('h,w,scale', [(97, 131, (1333, 800)), (1500, 2000, (1000, 600)), (333, 250, (333, 250)),
                                       (2, 3, (640, 480))])
def test_kernel_matches_restatement_upscale_and_downscale(h, w, scale):
    raw = _synthetic(h, w, h * 1000 + w)
    _check_separate(_transform(), [raw, raw], [scale, scale], [False, True])


@pytest.mark.parametrize('divisor', [32, None])
def test_kernel_matches_restatement_without_keep_ratio(divisor):
    raw = _synthetic(200, 300, 5)
    T = _transform(size_divisor=divisor)
    _check_separate(T, [raw] * 3, [(511, 77), (123, 456), (300, 200)], [False, True, False], keep_ratio=False)


@pytest.mark.parametrize('h,w', [(1, 1), (1, 9), (9, 1)])
def test_kernel_matches_restatement_on_degenerate_sources(h, w):
    raw = _synthetic(h, w, 11 + h + w)
    T = _transform(size_divisor=None)
    _check_separate(T, [raw] * 3, [(13, 5), (1, 1), (40, 24)], [False, True, True], keep_ratio=False)
    _check_separate(_transform(), [raw], [(40, 24)], [True], keep_ratio=True)


@pytest.mark.parametrize('new_w', [1, 3, 5, 1331])
@pytest.mark.parametrize('divisor', [None, 32])
def test_kernel_matches_restatement_for_widths_off_the_vector_grid(new_w, divisor):
    raw = _synthetic(50, 60, new_w)
    _check_separate(_transform(size_divisor=divisor), [raw, raw], [(new_w, 37), (new_w, 2)], [False, True],
                    keep_ratio=False)


def test_kernel_reads_a_padded_source_pitch_and_device_sources():
    big = _synthetic(120, 175, 3).cuda()
    raw = big[:, 5:165]                                           # row pitch 525 bytes, rows start 15 bytes in
    assert raw.stride(0) == 525 and not raw.is_contiguous()
    T = _transform()
    outs, _ = T.separate([raw, raw], [(400, 300), (400, 300)], [False, True])
    for o, flip in zip(outs, (False, True)):
        want = _restated(T, raw.contiguous(), (400, 300), flip)[0]
        assert torch.equal(o[0].cpu(), torch.from_numpy(want))


def test_kernel_channel_order_and_statistics():
    raw = _synthetic(211, 160, 4)
    mean, std = NORM['mean'], NORM['std']
    T = _transform(to_rgb=False, mean=mean[::-1], std=std[::-1])
    _check_separate(T, [raw, raw], [SCALES[1]] * 2, [False, True])
    bgr, _ = T([raw], [SCALES[1]], [False])
    rgb, _ = _transform()([raw], [SCALES[1]], [False])
    assert torch.equal(bgr.flip(1), rgb)
    other = _transform(mean=[0, 0, 0], std=[1, 1, 1])
    _check_separate(other, [raw], [SCALES[1]], [False])
    assert float(other([raw], [SCALES[1]], [False])[0].max()) > 200             # (its own table, not a cached one)


def test_mixed_size_batch_at_common_size_overwrites_every_element_of_out(demo_images):
    T = _transform()
    raws = [demo_images[0], demo_images[1], _synthetic(300, 700, 1), demo_images[3], _synthetic(64, 64, 2)]
    scales = [SCALES[0], SCALES[1], SCALES[0], SCALES[1], (96, 96)]
    flips = [False, True, True, False, True]
    pads = [preprocess.plan(r.shape[0], r.shape[1], s, True, 32)[3] for r, s in zip(raws, scales)]
    H, W = max(p[0] for p in pads), max(p[1] for p in pads)
    assert len(set(pads)) > 2
    with pytest.raises(ValueError):
        T(raws, scales, flips)                                    # different pad shapes need common_size
    out = torch.full((len(raws), 3, H, W), float('nan'), device='cuda')
    img, metas = T(raws, scales, flips, out=out, common_size=True)
    assert img is out
    host = out.cpu()
    assert not torch.isnan(host).any()
    for b, (r, s, f) in enumerate(zip(raws, scales, flips)):
        want, img_shape, pad_shape, sf = _restated(T, r, s, f, out_hw=(H, W))
        assert metas[b] == (img_shape, pad_shape, sf) and pad_shape == pads[b]
        assert torch.equal(host[b], torch.from_numpy(want)), b
    # an explicit common size, freshly allocated
    img2, _ = T(raws, scales, flips, common_size=(H + 32, W + 64))
    assert tuple(img2.shape) == (len(raws), 3, H + 32, W + 64)
    assert torch.equal(img2[:, :, :H, :W].cpu(), host) and not img2[:, :, H:].any() and not img2[:, :, :, W:].any()


@pytest.mark.parametrize('col0,width', [(1, 801), (2, 803), (3, 800), (0, 802)])
def test_out_views_off_the_16_byte_grid(col0, width):
    """destination rows that start 4 / 8 / 12 bytes off a 16-byte boundary, odd plane strides: the scalar head / tail and the
    all-scalar path write the same values, and nothing outside the view"""
    T = _transform()
    raws = [_synthetic(240, 320, 8), _synthetic(100, 150, 9)]
    scales, flips = [(400, 300), (400, 300)], [True, False]
    H = 321 if width % 2 else 320                                # (pad shapes 320 x 416 and 288 x 416)
    W = 416
    big = torch.full((2, 3, H, width), float('nan'), device='cuda')
    view = big[:, :, :, col0:col0 + W]
    T(raws, scales, flips, out=view, common_size=(H, W))
    host = big.cpu()
    for b in range(2):
        want = _restated(T, raws[b], scales[b], flips[b], out_hw=(H, W))[0]
        assert torch.equal(host[b, :, :, col0:col0 + W], torch.from_numpy(want))
    outside = torch.ones(width, dtype=torch.bool)
    outside[col0:col0 + W] = False
    assert torch.isnan(host[..., outside]).all()


def test_more_jobs_than_one_launch_holds():
    T = _transform()
    n = 2 * _lib.PREPROC_MAX_JOBS + 6
    raws = [_synthetic(20 + i % 7, 31 + i % 5, i) for i in range(n)]
    scales = [(64 + 8 * (i % 3), 48) for i in range(n)]
    flips = [bool(i % 2) for i in range(n)]
    _check_separate(T, raws, scales, flips)
    img, _ = T(raws, scales, flips, common_size=True)
    for b in (0, _lib.PREPROC_MAX_JOBS - 1, _lib.PREPROC_MAX_JOBS, n - 1):
        want = _restated(T, raws[b], scales[b], flips[b], out_hw=tuple(img.shape[2:]))[0]
        assert torch.equal(img[b].cpu(), torch.from_numpy(want))


# ---- C ABI -------------------------------------------------------------------------------------
def _job(src_t, dst_t, **kw):
    src, dst = src_t, dst_t
    f = dict(src=src.data_ptr(), src_h=src.shape[0], src_w=src.shape[1], src_row_bytes=src.stride(0), dst=dst.data_ptr(),
             dst_channel_stride=dst.stride(0), dst_row_stride=dst.stride(1), new_h=dst.shape[1], new_w=dst.shape[2],
             out_h=dst.shape[1], out_w=dst.shape[2], scale_y=float(preprocess.axis_scale(src.shape[0], dst.shape[1])),
             scale_x=float(preprocess.axis_scale(src.shape[1], dst.shape[2])), flip=0)
    f.update(kw)
    return _lib.PreprocJob(**f)


def _call(jobs, n, lut):
    L = _lib.lib()
    arr = (_lib.PreprocJob * max(len(jobs), 1))(*jobs)
    return L.kgdet_image_preprocess(arr, ctypes.c_int32(n), _lib.ptr(lut), ctypes.c_int32(0), _lib.current_stream())


def test_c_abi_limits_are_reported():
    L = _lib.lib()
    lut = torch.from_numpy(preprocess.norm_table(NORM['mean'], NORM['std'])).cuda()
    src = _synthetic(16, 24, 0).cuda()
    dst = torch.full((3, 8, 12), float('nan'), device='cuda')
    assert _call([], 0, lut) == _lib.KGDET_OK
    assert L.kgdet_image_preprocess(None, ctypes.c_int32(0), None, ctypes.c_int32(0), None) == _lib.KGDET_OK
    for bad in (dict(src_h=0), dict(src_w=-1), dict(new_h=0), dict(new_w=0), dict(out_w=11), dict(out_h=7),
                dict(src_row_bytes=71), dict(dst_row_stride=11), dict(dst_channel_stride=0), dict(scale_x=0.0),
                dict(scale_y=float('nan')), dict(src=0), dict(dst=0)):
        assert _call([_job(src, dst, **bad)], 1, lut) == _lib.KGDET_E_SHAPE, bad
        assert b'image_preprocess' in L.kgdet_last_error(), bad
    assert _call([_job(src, dst)], -1, lut) == _lib.KGDET_E_SHAPE
    many = [_job(src, dst)] * (_lib.PREPROC_MAX_JOBS + 1)
    assert _call(many, len(many), lut) == _lib.KGDET_E_UNSUPPORTED
    assert b'limit' in L.kgdet_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(dst).all()                                  # no rejected call wrote anything
    assert _call([_job(src, dst)], 1, lut) == _lib.KGDET_OK
    torch.cuda.synchronize()
    want = preprocess.image_transform_restatement(src.cpu().numpy(), (12, 8), False, False, NORM['mean'], NORM['std'])[0]
    assert torch.equal(dst.cpu(), torch.from_numpy(want))


# ---- end to end --------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def kgdet():
    _, model = demo_cases.demo_detector()
    return model.cuda().eval()


def _restatement_dataset(**kw):
    data = demo_cases.demo_dataset(test_mode=True, **kw)
    data.img_transform = preprocess.RestatementImageTransform(size_divisor=data.size_divisor, **data.img_norm_cfg)
    return data


def _assert_same_result(g, w, where, exact=True):
    """one image's result tuple: (per-class boxes, scores, per-class landmarks), or a 1-tuple when nothing was detected"""
    assert len(g) == len(w), where
    for part_g, part_w in zip(g, w):
        assert len(part_g) == len(part_w), where
        for x, y in zip(part_g, part_w):
            if exact:
                assert np.array_equal(x, y), where
            else:
                assert x.shape == y.shape and np.allclose(x, y, rtol=1e-5, atol=1e-3), where


def _assert_same_results(got, want, exact=True):
    assert len(got) == len(want) == 32
    for i, (g, w) in enumerate(zip(got, want)):
        _assert_same_result(g, w, i, exact)
    assert sum(len(r) == 3 for r in want) > 0


@pytest.mark.parametrize('imgs_per_gpu', [1, 8])
def test_single_gpu_test_with_device_preprocess_equals_restatement_inputs(kgdet, imgs_per_gpu):
    """the same input bits, a deterministic detector: the results are equal array for array"""
    to_dev = lambda t: t.cuda(non_blocking=True)
    # (a first pass over the shapes: the first forward at a new shape may pick other convolution algorithms)
    runner.single_gpu_test(kgdet, demo_cases.demo_dataset(test_mode=True), imgs_per_gpu=imgs_per_gpu, device_preprocess=True)
    want = runner.single_gpu_test(kgdet, _restatement_dataset(), to_device=to_dev, imgs_per_gpu=imgs_per_gpu)
    got = runner.single_gpu_test(kgdet, demo_cases.demo_dataset(test_mode=True), imgs_per_gpu=imgs_per_gpu,
                                 device_preprocess=True)
    _assert_same_results(got, want)


def test_single_gpu_test_with_device_preprocess_flip_and_two_scales(kgdet):
    """flip + two-scale TTA.  The INPUTS are equal bit for bit (all 32 samples, 4 augmentations each, one launch per sample).
    The results are compared with the tolerance of tests/test_gpu_aug_test.py's end-to-end test (rtol 1e-5, atol 1e-3),
    not exactly: measured on the MI355X, ``aug_candidates`` of the two-image (image + flip) batch at 800 x 608 is not
    repeatable run to run on IDENTICAL input tensors, with or without this route -- two passes of the host-transform path
    over the same samples differ from each other by up to 1.8e-4 in a coordinate (1e-7 in a score) on 3 of the first 8 demo
    images, exactly as the device route differs from the host route; the single-augmentation passes above are exact."""
    kw = dict(flip_ratio=0.5, img_scale=[(1333, 800), (1000, 600)])
    data, ref = demo_cases.demo_dataset(test_mode=True, **kw), _restatement_dataset(**kw)
    T = data.device_transform()
    for i in range(32):
        raw, r = data.prepare_test_raw(i), ref[i]
        imgs, _ = T.separate([raw['raw']] * 4, raw['scales'], raw['flips'], keep_ratio=raw['keep_ratio'])
        assert len(imgs) == len(r['img']) == 4
        for a, b, ma, mb in zip(imgs, r['img'], raw['img_meta'], r['img_meta']):
            assert torch.equal(a[0].cpu(), b)
            assert all(ma[k] == mb[k] for k in ('img_shape', 'pad_shape', 'scale_factor', 'flip', 'ori_shape'))
    to_dev = lambda t: t.cuda(non_blocking=True)
    runner.single_gpu_test(kgdet, data, device_preprocess=True)
    want = runner.single_gpu_test(kgdet, ref, to_device=to_dev)
    got = runner.single_gpu_test(kgdet, data, device_preprocess=True)
    _assert_same_results(got, want, exact=False)


def test_graphed_batches_written_into_static_img_leave_no_stale_padding(kgdet):
    """two different batches with the same metas, back to back through the graph's input buffer ``run.static_img`` (which
    holds NaN before the first and a batch that fills the whole slot before the second): each gives the results of
    ``simple_test_batch`` on its restatement input"""
    data = demo_cases.demo_dataset(test_mode=True)
    T = data.device_transform()
    same = [i for i, info in enumerate(data.img_infos) if (info['height'], info['width']) == (624, 468)]
    assert len(same) >= 4
    batches = [[data.prepare_test_raw(i) for i in same[:2]], [data.prepare_test_raw(i) for i in same[2:4]]]
    metas = [s['img_meta'][0] for s in batches[0]]
    pad = metas[0]['pad_shape']
    assert pad[0] > metas[0]['img_shape'][0]                      # (there are padding rows)
    for s, m in zip(batches[1], metas):
        assert all(s['img_meta'][0][k] == m[k] for k in ('img_shape', 'pad_shape', 'scale_factor', 'ori_shape'))

    def restated(batch):
        return torch.from_numpy(np.stack([_restated(T, s['raw'], s['scales'][0], False)[0] for s in batch])).cuda()

    def write(batch, keep_ratio=True, scale=None):
        T([s['raw'] for s in batch], [scale or s['scales'][0] for s in batch], [False] * len(batch), keep_ratio=keep_ratio,
          out=run.static_img)

    run = kgdet.graphed_test_batch(restated(batches[0]), metas, rescale=True)
    run.static_img.fill_(float('nan'))
    seen = []
    for k, batch in enumerate(batches):
        if k:
            write(batches[0], keep_ratio=False, scale=(pad[1], pad[0]))      # every element of the buffer non-zero pixels
            assert int((run.static_img[:, :, metas[0]['img_shape'][0]:] != 0).sum()) > 0
        write(batch)
        assert torch.equal(run.static_img, restated(batch))
        got = run(run.static_img)
        with torch.no_grad():
            want = kgdet.simple_test_batch(restated(batch), metas, rescale=True)
        assert len(got) == len(want) == 2 and sum(len(d) for r in want for d in r[0]) > 0
        for b, (g, w) in enumerate(zip(got, want)):
            _assert_same_result(g, w, (k, b))
        seen.append(want)
    assert not all(np.array_equal(x, y) for x, y in zip(seen[0][0][0], seen[1][0][0]))       # (the batches do differ)


def test_collate_device_equals_collate_of_restatement_samples_and_trains(kgdet):
    kw = dict(test_mode=False, flip_ratio=0.5, img_scale=[(1333, 800), (1000, 600)])
    data = demo_cases.demo_dataset(**kw)
    ref = demo_cases.demo_dataset(**kw)
    ref.img_transform = preprocess.RestatementImageTransform(size_divisor=ref.size_divisor, **ref.img_norm_cfg)
    idx = [0, 3, 5, 6]
    np.random.seed(77)
    want = datasets.collate([ref.prepare_train_img(i) for i in idx])
    np.random.seed(77)
    samples = [data.prepare_train_raw(i) for i in idx]
    got = datasets.collate_device(samples, data.device_transform())
    assert len({s['img_meta']['pad_shape'] for s in samples}) > 1               # (a mixed batch: the common size pads)
    assert set(got) == set(want)
    assert got['img'].is_cuda and torch.equal(got['img'].cpu(), want['img'])
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
