"""Fixture generation (build container only): tests/golden/extra_aug_golden.npz -- the reference's own
``mmdet/datasets/extra_aug.py`` (with its ``mmdet/core/evaluation/bbox_overlaps.py``) executed IN PLACE, loaded by path, on
committed seeds over small inputs.  Nothing of the reference's text is copied.

mmcv / cv2 are not available, so ``mmcv.bgr2hsv`` / ``mmcv.hsv2bgr`` are stubbed with the IDENTITY: the fixture pins everything
around the two conversions -- the order and kind of the draws, the order of the arithmetic, the ``int()`` places, the quirks of
``RandomCrop`` -- and leaves the conversions themselves to tests/test_augment.py's colorsys check.  With the identity the
"saturation" factor multiplies channel 1 (G) and the "hue" delta is added to channel 0 (B) of the reference's BGR image.

Per case: the uint8 BGR input, boxes, labels, the seed -> the output image (float32 BGR), boxes, labels, and one more draw
from the global RNG after the call (it pins the NUMBER of draws).

python tests/golden/make_extra_aug_golden.py"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/mmdetection/mmdet'
OUT = os.path.join(HERE, 'extra_aug_golden.npz')

MEAN = (123.675, 116.28, 103.53)
CONFIGS = {
    'photo': dict(photo_metric_distortion=dict(brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5),
                                               hue_delta=18)),
    'expand': dict(expand=dict(mean=MEAN, to_rgb=True, ratio_range=(1, 3))),
    'crop': dict(random_crop=dict(min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.3)),
    'all': dict(photo_metric_distortion=dict(brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5),
                                             hue_delta=18),
                expand=dict(mean=MEAN, to_rgb=False, ratio_range=(1, 4)),
                random_crop=dict(min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.3)),
}
SEEDS = range(6)
H, W = 12, 18


def case_input(name, seed):
    """the committed inputs of one case (tests regenerate nothing: they read these from the .npz)"""
    rng = np.random.default_rng(1000 * sorted(CONFIGS).index(name) + seed)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    n = 1 + seed % 4
    x1 = rng.uniform(0, W - 6, n)
    y1 = rng.uniform(0, H - 5, n)
    boxes = np.stack([x1, y1, x1 + rng.uniform(3, W - 1 - x1), y1 + rng.uniform(3, H - 1 - y1)], axis=1).astype(np.float32)
    labels = rng.integers(1, 14, n).astype(np.int64)
    return img, boxes, labels


def load_reference():
    def by_path(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    mmcv = types.ModuleType('mmcv')
    mmcv.bgr2hsv = lambda img: img
    mmcv.hsv2bgr = lambda img: img
    sys.modules['mmcv'] = mmcv
    for name in ('mmdet', 'mmdet.core', 'mmdet.core.evaluation'):
        sys.modules.setdefault(name, types.ModuleType(name))
    by_path('mmdet.core.evaluation.bbox_overlaps', os.path.join(REF, 'core', 'evaluation', 'bbox_overlaps.py'))
    return by_path('ref_extra_aug', os.path.join(REF, 'datasets', 'extra_aug.py'))


def main():
    ref = load_reference()
    out = {}
    for name, cfg in sorted(CONFIGS.items()):
        aug = ref.ExtraAugmentation(**cfg)
        for seed in SEEDS:
            img, boxes, labels = case_input(name, seed)
            np.random.seed(seed)
            o_img, o_boxes, o_labels = aug(img.copy(), boxes.copy(), labels.copy())
            key = '%s_%d_' % (name, seed)
            out[key + 'img'], out[key + 'boxes'], out[key + 'labels'] = img, boxes, labels
            out[key + 'out_img'] = np.ascontiguousarray(o_img)
            out[key + 'out_boxes'], out[key + 'out_labels'] = np.array(o_boxes), np.array(o_labels)
            out[key + 'next_draw'] = np.array(np.random.randint(1 << 30))
            assert o_img.dtype == np.float32 and out[key + 'out_boxes'].dtype == np.float32
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
