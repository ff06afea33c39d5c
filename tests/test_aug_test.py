"""Test-time augmentation on the host: the restatement ``detector.merge_aug_results_kp`` (flip undone, scale divided out,
augmentations concatenated) in closed form and as the inverse of the transforms the dataset applies."""
import os

import numpy as np
import pytest
import torch

from kgdet_amd import datasets as ds
from kgdet_amd.detector import merge_aug_results_kp, rescale_aug_detections
from kgdet_amd.postprocess import flip_perm

HERE = os.path.dirname(os.path.abspath(__file__))
ANN = os.path.join(HERE, 'golden', 'demo_dataset-32.json')
NORM = dict(mean=[154.992, 146.197, 140.744], std=[62.757, 64.507, 62.076], to_rgb=True)


def _dataset():
    return ds.DeepFashion2Dataset(ann_file=ANN, img_prefix='/nonexistent/', img_scale=(1333, 800), img_norm_cfg=NORM,
                                  size_divisor=32, flip_ratio=0.5, with_keypoint=True, with_mask=False, with_crowd=False,
                                  with_label=True, test_mode=True)


def _meta(data, img_shape, sf, flip):
    return dict(img_shape=img_shape, scale_factor=sf, flip=flip, flip_indices=data.flip_indices)


def test_closed_form_flip_and_scale():
    data = _dataset()
    K = 294
    perm = data.flip_indices[0::2] // 2
    k = int(np.nonzero(perm != np.arange(K))[0][0])           # a landmark with a left/right partner
    partner = int(perm[k])
    boxes = torch.tensor([[10., 20., 30., 40.]])
    scores = torch.tensor([[0., 0.25, 0.75]])
    kpts = torch.zeros(1, K, 3)
    kpts[0, k] = torch.tensor([12., 14., 1.])
    kpts[0, partner] = torch.tensor([50., 60., 0.5])
    flipped = _meta(data, (80, 100, 3), 2.0, True)
    plain = _meta(data, (80, 100, 3), 2.0, False)
    b, s, kp = merge_aug_results_kp([boxes, boxes * 4], [scores, scores + 1], [kpts, kpts], [flipped, plain])
    assert b.shape == (2, 4) and s.shape == (2, 3) and kp.shape == (2, K, 3)
    # augmentation-major rows: the flipped one first, then the unflipped one
    assert b[0].tolist() == [34.5, 10.0, 44.5, 20.0]
    assert b[1].tolist() == [20.0, 40.0, 60.0, 80.0]
    assert torch.equal(s, torch.cat([scores, scores + 1]))
    # mirrored, moved to the partner slot, visibility untouched
    assert kp[0, partner].tolist() == [(100 - 12 - 1) / 2, 7.0, 1.0]
    assert kp[0, k].tolist() == [(100 - 50 - 1) / 2, 30.0, 0.5]
    untouched = [i for i in range(K) if i not in (k, partner)]
    assert kp[0, untouched, 0].eq(99 / 2).all() and kp[0, untouched, 1:].eq(0).all()
    # an unflipped augmentation is only divided
    assert torch.equal(kp[1], torch.cat([kpts[0, :, :2] / 2, kpts[0, :, 2:]], -1))


def test_empty_augmentation_and_flat_landmarks():
    data = _dataset()
    boxes = torch.tensor([[1., 2., 3., 4.]])
    kpts = torch.arange(294 * 3, dtype=torch.float32).reshape(1, 294 * 3)       # [n, 3K] is accepted too
    metas = [_meta(data, (50, 60, 3), 1.5, True), _meta(data, (50, 60, 3), 1.5, False)]
    b, s, kp = merge_aug_results_kp([torch.zeros(0, 4), boxes], [torch.zeros(0, 3), torch.ones(1, 3)],
                                    [torch.zeros(0, 294, 3), kpts], metas)
    assert b.shape == (1, 4) and kp.shape == (1, 294, 3)
    assert torch.equal(b, boxes / 1.5)


def test_non_scalar_scale_factor_is_refused():
    data = _dataset()
    meta = _meta(data, (50, 60, 3), np.array([1.5, 1.2, 1.5, 1.2], np.float32), False)
    with pytest.raises(NotImplementedError, match='scalar scale_factor'):
        merge_aug_results_kp([torch.zeros(1, 4)], [torch.zeros(1, 3)], [torch.zeros(1, 294, 3)], [meta])


def test_flip_perm_is_the_dataset_involution():
    data = _dataset()
    p = flip_perm(data.flip_indices, 'cpu')
    assert torch.equal(p[p], torch.arange(294))
    assert flip_perm(data.flip_indices, 'cpu') is p                      # cached
    with pytest.raises(ValueError):
        flip_perm(np.zeros(588, np.int64), 'cpu')


def test_round_trip_through_dataset_transforms():
    """ground truth of the demo annotations -> the dataset's own resize + flip -> mapped back: the originals"""
    data = _dataset()
    checked = 0
    for idx in range(len(data)):
        info, ann = data.img_infos[idx], data.get_ann_info(idx)
        if ann['bboxes'].shape[0] == 0 or len(ann['keypoints']) != ann['bboxes'].shape[0]:
            continue
        h, w, sf = ds.rescale_size(info['height'], info['width'], (1333, 800))
        shape = (h, w, 3)
        gt = ann['bboxes'].astype(np.float32)
        gt_kp = np.stack(ann['keypoints']).astype(np.float32)
        if not (gt[:, 2] * sf <= w - 1).all() or not (gt[:, 3] * sf <= h - 1).all():
            continue                                                     # (the transform clips; not invertible)
        fb = ds.bbox_transform(gt, shape, sf, flip=True).astype(np.float32)
        fk = ds.keypoint_transform(ann['keypoints'], shape, ann['labels'], sf, data.flip_pairs, flip=True)
        pb = ds.bbox_transform(gt, shape, sf, flip=False).astype(np.float32)
        pk = ds.keypoint_transform(ann['keypoints'], shape, ann['labels'], sf, data.flip_pairs, flip=False)
        n = gt.shape[0]
        b, s, k = merge_aug_results_kp(
            [torch.from_numpy(fb), torch.from_numpy(pb)], [torch.zeros(n, 14), torch.zeros(n, 14)],
            [torch.from_numpy(fk.astype(np.float32)), torch.from_numpy(pk.astype(np.float32))],
            [_meta(data, shape, sf, True), _meta(data, shape, sf, False)])
        for part in (slice(0, n), slice(n, 2 * n)):
            np.testing.assert_allclose(b[part].numpy(), gt, rtol=1e-5, atol=1e-3)
            np.testing.assert_allclose(k[part].numpy(), gt_kp, rtol=1e-5, atol=1e-3)
        checked += 1
    assert checked >= 16


def test_rescale_false_multiplies_by_first_scale():
    det = torch.tensor([[2., 4., 6., 8., 0.5]])
    kp = torch.tensor([[1., 2., 0.3] * 294])
    meta = dict(scale_factor=1.5)
    d, lab, k = rescale_aug_detections(det, torch.tensor([3]), kp, meta, rescale=False)
    assert d.tolist() == [[3., 6., 9., 12., 0.5]]
    assert k.shape == kp.shape and k[0, :3].tolist() == [1.5, 3., pytest.approx(0.3)]
    assert rescale_aug_detections(det, torch.tensor([3]), kp, meta, rescale=True)[0] is det
