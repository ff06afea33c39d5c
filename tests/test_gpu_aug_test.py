"""Test-time augmentation on the GPU: the merge kernel (csrc/aug_merge.hip) bit-exact against the restatement
``detector.merge_aug_results_kp``, the fused hard NMS in its widened envelope, ``RepPointsDetectorKp.aug_test`` for both head
families, and the demo set end to end through ``runner.single_gpu_test`` with flip and multi-scale test pipelines."""
import numpy as np
import pytest
import torch

from kgdet_amd import configs
from kgdet_amd.detector import merge_aug_results_kp, rescale_aug_detections
from kgdet_amd.postprocess import (aug_merge_kp, multiclass_nms_fused_supported, multiclass_nms_kp,
                                   multiclass_nms_kp_batched, multiclass_nms_kp_fused)
from tests.golden import demo_cases

pytestmark = pytest.mark.gpu

K, C = 294, 13


def _flip_indices():
    return demo_cases.demo_dataset(test_mode=True).flip_indices


def _candidates(n, w, h, gen):
    """decoded candidates of one augmentation as the heads produce them: clamped to [0, img_shape], some exactly at 0 / w"""
    boxes = torch.rand(n, 4, generator=gen) * torch.tensor([w, h, w, h]) * 1.2 - 5
    boxes = torch.stack([boxes[:, 0].clamp(0, w), boxes[:, 1].clamp(0, h), boxes[:, 2].clamp(0, w),
                         boxes[:, 3].clamp(0, h)], 1)
    scores = torch.cat([torch.zeros(n, 1), torch.rand(n, C, generator=gen)], 1)
    kpts = torch.rand(n, K, 3, generator=gen) * torch.tensor([w * 1.2, h * 1.2, 1.0]) - torch.tensor([3.0, 3.0, 0.0])
    kpts[..., 0] = kpts[..., 0].clamp(0, w)
    kpts[..., 1] = kpts[..., 1].clamp(0, h)
    if n:
        boxes[0] = torch.tensor([0.0, 0.0, w, h])
        kpts[0, :, 0] = w
        kpts[min(1, n - 1), :, 0] = 0
    return boxes.cuda(), scores.cuda(), kpts.cuda()


@pytest.mark.parametrize('plan', [
    [(1000, 1333, 800, 1.6660, True)],
    [(1000, 1333, 800, 1.6660, False), (608, 1333, 800, 1.6660, True)],
    [(1000, 1333, 800, 1.6660, False), (0, 1333, 800, 1.6660, True), (7, 1000, 600, 1.2495, True),
     (608, 1000, 600, 1.2495, False)],
    [(608, 1333, 800, 2.0, True), (1000, 1333, 800, 2.0, False), (1000, 999, 601, 0.75, True),
     (0, 999, 601, 0.75, False)],
])
def test_aug_merge_kernel_matches_restatement_bitwise(plan):
    gen = torch.Generator().manual_seed(len(plan))
    fi = _flip_indices()
    cands, metas = [], []
    for n, w, h, sf, flip in plan:
        cands.append(_candidates(n, w, h, gen))
        metas.append(dict(img_shape=(h, w, 3), scale_factor=sf, flip=flip, flip_indices=fi))
    got = aug_merge_kp([c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands], metas)
    want = merge_aug_results_kp([c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands], metas)
    T = sum(p[0] for p in plan)
    for g, r in zip(got, want):
        assert g.shape[0] == T and g.shape == r.shape
        assert torch.equal(g, r), (g - r).abs().max()


def test_aug_merge_rejects_more_than_16_augmentations():
    gen = torch.Generator().manual_seed(0)
    b, s, k = _candidates(3, 100, 80, gen)
    metas = [dict(img_shape=(80, 100, 3), scale_factor=1.0, flip=False, flip_indices=None)] * 17
    with pytest.raises(NotImplementedError):
        aug_merge_kp([b] * 17, [s] * 17, [k] * 17, metas)
    out = aug_merge_kp([b] * 16, [s] * 16, [k] * 16, metas[:16])
    assert out[0].shape == (48, 4)


def test_fused_nms_supported_envelope():
    assert multiclass_nms_fused_supported(1, 4096, 13, 100)
    assert not multiclass_nms_fused_supported(1, 4097, 13, 100)
    assert not multiclass_nms_fused_supported(1, 4096, 13, 1261)           # 13 * 1261 > 16384
    assert not multiclass_nms_fused_supported(1, 4096, 65, 100)
    assert multiclass_nms_fused_supported(1, 1000, 13, 2000)               # (the old envelope, N * C <= 16384)


@pytest.mark.parametrize('T', [2000, 4000])
def test_fused_nms_in_the_wider_envelope(T):
    gen = torch.Generator().manual_seed(T)
    centres = torch.rand(40, 2, generator=gen) * 700
    pick = torch.randint(0, 40, (T, ), generator=gen)
    wh = 40 + torch.rand(T, 2, generator=gen) * 30
    xy = centres[pick] + torch.randn(T, 2, generator=gen) * 4             # heavy overlaps around 40 centres
    boxes = torch.cat([xy - wh / 2, xy + wh / 2], 1).clamp(0, 800).cuda()
    scores = (torch.randint(0, 20, (T, C), generator=gen).float() / 20).cuda()   # many exactly tied scores
    scores = torch.cat([torch.zeros(T, 1, device='cuda'), scores], 1)
    kpts = torch.randn(T, 3 * K, generator=gen).cuda()
    assert multiclass_nms_fused_supported(1, T, C, 100)
    det, lab, kp, cnt = multiclass_nms_kp_fused(boxes[None], scores[None, :, 1:], kpts[None], 0.05, 0.5, 100)
    n = int(cnt[0])
    assert n == 100
    bd, bl, bk = multiclass_nms_kp_batched(boxes[None], scores[None], kpts[None], 0.05, dict(type='nms', iou_thr=0.5),
                                           100)[0]
    rd, rl, rk = multiclass_nms_kp(boxes, scores, kpts, 0.05, dict(type='nms', iou_thr=0.5), 100)
    for a, b, c in ((det[0, :n], bd, rd), (lab[0, :n], bl, rl), (kp[0, :n], bk, rk)):
        assert torch.equal(a, b) and torch.equal(a, c)


# ----------------------------------------------------------------------------------------------
def _restated(model, cands, img_metas, rescale):
    """steps 2-6 of aug_test on the restatement (pure torch merge, the per-class NMS loop)"""
    metas = [m[0] for m in img_metas]
    b, s, k = merge_aug_results_kp([c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands], metas)
    cfg = model.test_cfg
    det, lab, kp = multiclass_nms_kp(b, s, k.reshape(k.shape[0], -1), cfg.score_thr, cfg.nms, cfg.max_per_img)
    det, lab, kp = rescale_aug_detections(det, lab, kp, metas[0], rescale)
    return model.bbox2result_kp(det, lab, kp, model.bbox_head.num_classes)


def _assert_same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, list):
            assert len(x) == len(y) and all(np.array_equal(u, v) for u, v in zip(x, y))
        else:
            assert np.array_equal(x, y)


def _sample(data, idx):
    d = data[idx]
    return [t[None].cuda() for t in d['img']], [[m] for m in d['img_meta']]


@pytest.fixture(scope='module')
def kgdet():
    cfg, model = demo_cases.demo_detector()
    return model.cuda().eval()


def test_kgdet_flip_aug_test_matches_restatement(kgdet):
    data = demo_cases.demo_dataset(test_mode=True, flip_ratio=0.5)
    imgs, metas = _sample(data, 3)
    assert [m[0]['flip'] for m in metas] == [False, True]
    with torch.no_grad():
        res = kgdet.aug_test(imgs, metas, rescale=True)
        cands = kgdet.aug_candidates(imgs, metas)
        want = _restated(kgdet, cands, metas, rescale=True)
        via_forward = kgdet(imgs, metas, return_loss=False, rescale=True)
    assert len(res) == 3 and sum(len(x) for x in res[0]) > 0
    _assert_same(res, want)
    _assert_same(via_forward, want)


def test_kgdet_identity_augmentations_equal_simple_test(kgdet):
    data = demo_cases.demo_dataset(test_mode=True)
    imgs, metas = _sample(data, 5)
    with torch.no_grad():
        ref = kgdet.simple_test(imgs[0], metas[0], rescale=True)
        one = kgdet.aug_test(imgs, metas, rescale=True)
        two = kgdet.aug_test(imgs * 2, metas * 2, rescale=True)       # exact duplicates: IoU 1, NMS removes them
        unscaled = kgdet.aug_test(imgs * 2, metas * 2, rescale=False)
    assert len(ref) == 3
    for got in (one, two):
        assert len(got) == 3
        for cls in range(len(ref[0])):
            assert got[0][cls].shape == ref[0][cls].shape
            np.testing.assert_allclose(got[0][cls], ref[0][cls], rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(got[2][cls], ref[2][cls], rtol=1e-5, atol=1e-4)
    sf = metas[0][0]['scale_factor']
    for cls in range(len(ref[0])):
        np.testing.assert_allclose(unscaled[0][cls][:, :4], two[0][cls][:, :4] * sf, rtol=1e-6, atol=1e-4)
        assert np.array_equal(unscaled[0][cls][:, 4], two[0][cls][:, 4])
        k_u, k_r = unscaled[2][cls].reshape(-1, K, 3), two[2][cls].reshape(-1, K, 3)
        np.testing.assert_allclose(k_u[..., :2], k_r[..., :2] * sf, rtol=1e-6, atol=1e-4)
        assert np.array_equal(k_u[..., 2], k_r[..., 2])


@pytest.mark.parametrize('soft', [False, True])
def test_serial_detector_two_scales_and_flip_match_restatement(soft):
    from kgdet_amd.registry import build_detector
    cfg = configs.reppoints_kp_r50_fpn(soft_nms=soft)
    torch.manual_seed(0)
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda().eval()
    model.bbox_head.cls_refine_out.bias.data.fill_(-2.0)          # scores above score_thr for the random weights
    fi = _flip_indices()
    gen = torch.Generator().manual_seed(7)
    imgs, metas = [], []
    # hard NMS: 4900 merged candidates, beyond the fused NMS (batched path); soft-NMS: 3708, the fused soft-NMS (the
    # per-class soft_nms op of the restatement takes at most 4544 boxes of a class)
    second = ((128, 160), 0.2) if soft else ((192, 256), 0.3)
    for (h, w), sf in (((256, 320), 0.4), second):
        x = torch.randn(1, 3, h, w, generator=gen).cuda()
        for flip in (False, True):
            imgs.append(torch.flip(x, [3]) if flip else x)
            metas.append([dict(img_shape=(h, w, 3), pad_shape=(h, w, 3), ori_shape=(640, 800, 3), scale_factor=sf,
                               flip=flip, flip_indices=fi)])
    with torch.no_grad():
        cands = model.aug_candidates(imgs, metas)
        got = model.bbox2result_kp(*model.merge_aug_detections(cands, metas, rescale=True), model.bbox_head.num_classes)
        want = _restated(model, cands, metas, rescale=True)
        res = model.aug_test(imgs, metas, rescale=True)
    assert sum(c[0].shape[0] for c in cands) == (3708 if soft else 4900)
    assert len(want) == 3
    _assert_same(got, want)
    assert len(res) == 3                                        # (a second forward pass: same detections)
    for x, y in zip(res[0], want[0]):
        assert x.shape == y.shape and np.allclose(x, y, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize('scales', [None, [(1333, 800), (1000, 600)]])
def test_demo_set_tta_end_to_end(kgdet, scales, tmp_path):
    from kgdet_amd import evaluation, runner
    kw = dict(flip_ratio=0.5)
    if scales is not None:
        kw['img_scale'] = scales
    data = demo_cases.demo_dataset(test_mode=True, **kw)
    results = runner.single_gpu_test(kgdet, data, rescale=True, to_device=lambda t: t.cuda(non_blocking=True))
    assert len(results) == len(data) == 32
    with torch.no_grad():
        for i, r in enumerate(results):
            imgs, metas = _sample(data, i)
            assert len(imgs) == (4 if scales else 2)
            # (a second forward pass of the image: the first pass at a new shape may pick other convolution algorithms)
            want = _restated(kgdet, kgdet.aug_candidates(imgs, metas), metas, rescale=True)
            assert len(r) == len(want)
            if len(want) == 3:
                for x, y in zip(r[0] + r[2], want[0] + want[2]):
                    assert x.shape == y.shape and np.allclose(x, y, rtol=1e-5, atol=1e-3), i
    assert sum(len(r) == 3 for r in results) > 0
    files = evaluation.results2json(data, results, str(tmp_path / 'tta'))
    stats = evaluation.coco_eval(files, ['bbox', 'keypoints'], data.coco, verbose=False)
    for typ in ('bbox', 'keypoints'):
        assert np.isfinite(stats[typ][0]), (typ, stats[typ])
