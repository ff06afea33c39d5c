"""Train-time ``extra_aug`` (``mmdet/datasets/extra_aug.py``): photometric distortion, expand, random crop -- the DRAWS and
the ground truth, on the host, in numpy.  No pixel is touched here.

``ExtraAugmentation(photo_metric_distortion, expand, random_crop).draw(h, w, boxes, labels)`` makes the reference's draws from
numpy's global RNG -- in its order and of its kind (``randint(2)``, ``uniform``, ``permutation(3)``, ``choice``), so one seed
gives the reference's decisions -- and returns an ``AugPlan``.  The pixels follow from the plan alone:
``preprocess.image_transform_restatement_aug`` on the host, ``csrc/preprocess_aug.hip`` on the device (the distortion on every
source pixel, expand and crop as a window in front of the resize).  ``AugPlan.apply_gt`` moves the ground truth.

Where this differs from the reference, on purpose:

* the reference's ``ExtraAugmentation`` passes ``(img, boxes, labels)`` only, so ``Expand`` and ``RandomCrop`` leave the
  landmarks and the ignore boxes where they were; ``apply_gt`` carries both along.
* the reference's ``boxes +=`` / ``boxes -=`` edit the annotation arrays in place; everything here works on copies.
* the reference's image is BGR, this project's RGB: a drawn channel permutation ``p`` (``new_bgr[i] = bgr[p[i]]``) acts on
  RGB as ``q[j] = 2 - p[2 - j]``, and the expand fill is kept in RGB order.
"""
import numpy as np
from numpy import random


def bbox_overlaps(bboxes1, bboxes2):
    """IoU [n, k] of two box arrays: ``mmdet/core/evaluation/bbox_overlaps.py`` (mode 'iou') restated -- float32
    throughout, extents with ``+ 1``, the loop over the SHORTER array (the result is transposed back)."""
    bboxes1 = bboxes1.astype(np.float32)
    bboxes2 = bboxes2.astype(np.float32)
    rows, cols = bboxes1.shape[0], bboxes2.shape[0]
    ious = np.zeros((rows, cols), dtype=np.float32)
    if rows * cols == 0:
        return ious
    exchange = rows > cols
    if exchange:
        bboxes1, bboxes2 = bboxes2, bboxes1
        ious = np.zeros((cols, rows), dtype=np.float32)
    area1 = (bboxes1[:, 2] - bboxes1[:, 0] + 1) * (bboxes1[:, 3] - bboxes1[:, 1] + 1)
    area2 = (bboxes2[:, 2] - bboxes2[:, 0] + 1) * (bboxes2[:, 3] - bboxes2[:, 1] + 1)
    for i in range(bboxes1.shape[0]):
        x_start = np.maximum(bboxes1[i, 0], bboxes2[:, 0])
        y_start = np.maximum(bboxes1[i, 1], bboxes2[:, 1])
        x_end = np.minimum(bboxes1[i, 2], bboxes2[:, 2])
        y_end = np.minimum(bboxes1[i, 3], bboxes2[:, 3])
        overlap = np.maximum(x_end - x_start + 1, 0) * np.maximum(y_end - y_start + 1, 0)
        ious[i, :] = overlap / (area1[i] + area2 - overlap)
    return ious.T if exchange else ious


def rgb_permutation(p):
    """the drawn BGR permutation ``p`` (``new_bgr[i] = bgr[p[i]]``) on RGB order: ``q[j] = 2 - p[2 - j]``"""
    return tuple(2 - int(p[2 - j]) for j in range(3))


class AugPlan(object):
    """The decisions of one ``ExtraAugmentation`` call on an ``h x w`` image.

    colour -- ``colour``: photometric distortion is configured (the HSV round trip runs even with every draw off);
      ``delta`` / ``alpha`` / ``sat`` / ``hue``: the drawn brightness delta, contrast factor, saturation factor and hue delta,
      ``None`` where the coin said no; ``contrast_first``: the contrast multiplies before the HSV stage; ``perm``: the drawn
      BGR channel permutation or ``None`` (``q`` is its RGB form).
    expand -- ``canvas``: (H, W) or ``None``; ``top`` / ``left``: the image's place in it; ``fill``: the canvas colour in RGB
      order, float32 [3] (``None``: the normalisation mean, which the pixel routes substitute).
    crop -- ``patch``: (x1, y1, x2, y2) in canvas coordinates or ``None``; ``keep``: the kept-box mask (all true without a crop).
    """

    def __init__(self, h, w, n_boxes):
        self.h, self.w = int(h), int(w)
        self.colour = False
        self.delta = self.alpha = self.sat = self.hue = self.perm = None
        self.contrast_first = False
        self.canvas, self.top, self.left, self.fill = None, 0, 0, None
        self.patch = None
        self.keep = np.ones(n_boxes, dtype=bool)

    @property
    def q(self):
        return None if self.perm is None else rgb_permutation(self.perm)

    @property
    def canvas_hw(self):
        return (self.h, self.w) if self.canvas is None else self.canvas

    @property
    def virtual_hw(self):
        """(vh, vw): the size of the image the resize reads -- the patch, else the canvas, else the raw image"""
        if self.patch is None:
            return self.canvas_hw
        return self.patch[3] - self.patch[1], self.patch[2] - self.patch[0]

    @property
    def origin(self):
        """(oy, ox): where raw pixel (0, 0) sits in the virtual image; negative when the crop cuts into the raw image"""
        x1, y1 = (0, 0) if self.patch is None else self.patch[:2]
        return self.top - y1, self.left - x1

    def is_identity(self):
        return not self.colour and self.canvas is None and self.patch is None

    def apply_gt(self, boxes, labels, keypoints=None, boxes_ignore=None):
        """the ground truth in the virtual image's coordinates -> (boxes, labels, keypoints, boxes_ignore), all new arrays.

        boxes exactly as the reference leaves them: + (left, top), the centre mask, clipped to the patch, - the patch
        origin; labels and landmark rows by the same mask.  A labelled landmark (v != 0) is shifted by the same two offsets
        and becomes (0, 0, 0) -- DeepFashion2's unlabelled landmark, weight 0 in ``points.py`` -- when it leaves
        [0, patch_w) x [0, patch_h); ignore boxes are shifted, clipped to the patch and dropped when nothing of them is
        left (both beyond the reference, which moves neither)."""
        shift = np.tile((self.left, self.top), 2).astype(np.float32)
        boxes = np.array(boxes, dtype=np.float32).reshape(-1, 4) + shift
        labels = np.array(labels)
        assert len(boxes) == len(self.keep) == len(labels)
        ignore = None if boxes_ignore is None else np.array(boxes_ignore, dtype=np.float32).reshape(-1, 4) + shift
        vh, vw = self.virtual_hw
        if self.patch is not None:
            patch = np.array(self.patch)
            boxes, labels = boxes[self.keep], labels[self.keep]
            boxes[:, 2:] = boxes[:, 2:].clip(max=patch[2:])
            boxes[:, :2] = boxes[:, :2].clip(min=patch[:2])
            boxes -= np.tile(patch[:2], 2).astype(np.float32)
            if ignore is not None:
                left_over = ((ignore[:, 0] < patch[2]) & (ignore[:, 2] >= patch[0])
                             & (ignore[:, 1] < patch[3]) & (ignore[:, 3] >= patch[1]))
                ignore = ignore[left_over]
                ignore[:, 2:] = ignore[:, 2:].clip(max=patch[2:])
                ignore[:, :2] = ignore[:, :2].clip(min=patch[:2])
                ignore -= np.tile(patch[:2], 2).astype(np.float32)
        out_kps = None
        if keypoints is not None:
            oy, ox = self.origin
            out_kps = []
            for kp, kept in zip(keypoints, self.keep):       # (rows beyond the boxes -- crowd annotations -- have no mask)
                if not kept:
                    continue
                kp = np.array(kp, dtype=np.float64).reshape(-1, 3)
                on = kp[:, 2] != 0
                kp[on, 0] += ox
                kp[on, 1] += oy
                gone = on & ~((kp[:, 0] >= 0) & (kp[:, 0] < vw) & (kp[:, 1] >= 0) & (kp[:, 1] < vh))
                kp[gone] = 0
                out_kps.append(kp)
        return boxes, labels, out_kps, ignore


class PhotoMetricDistortion(object):
    def __init__(self, brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18):
        self.brightness_delta = brightness_delta
        self.contrast_lower, self.contrast_upper = contrast_range
        self.saturation_lower, self.saturation_upper = saturation_range
        self.hue_delta = hue_delta

    def draw(self, plan):
        plan.colour = True
        if random.randint(2):
            plan.delta = random.uniform(-self.brightness_delta, self.brightness_delta)
        # quirk: the reference's comment says "mode == 0 --> contrast first"; its code multiplies BEFORE the HSV stage when
        # mode == 1, and the code is what runs
        mode = random.randint(2)
        if mode == 1:
            plan.contrast_first = True
            if random.randint(2):
                plan.alpha = random.uniform(self.contrast_lower, self.contrast_upper)
        if random.randint(2):
            plan.sat = random.uniform(self.saturation_lower, self.saturation_upper)
        if random.randint(2):
            plan.hue = random.uniform(-self.hue_delta, self.hue_delta)
        if mode == 0:
            if random.randint(2):
                plan.alpha = random.uniform(self.contrast_lower, self.contrast_upper)
        if random.randint(2):
            plan.perm = tuple(int(i) for i in random.permutation(3))


class Expand(object):
    def __init__(self, mean=(0, 0, 0), to_rgb=True, ratio_range=(1, 4)):
        # the reference keeps the fill in ITS image's order (BGR): mean[::-1] if to_rgb else mean.  In RGB order that is:
        self.fill = np.array(mean if to_rgb else mean[::-1], dtype=np.float32)
        self.min_ratio, self.max_ratio = ratio_range

    def draw(self, plan):
        if random.randint(2):                      # (1 = leave the image alone)
            return
        h, w = plan.h, plan.w
        ratio = random.uniform(self.min_ratio, self.max_ratio)
        plan.canvas = (int(h * ratio), int(w * ratio))
        plan.left = int(random.uniform(0, w * ratio - w))
        plan.top = int(random.uniform(0, h * ratio - h))
        plan.fill = self.fill.copy()


class RandomCrop(object):
    def __init__(self, min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.3):
        self.sample_mode = (1,) + tuple(min_ious) + (0,)       # 1: return the image as it is
        self.min_crop_size = min_crop_size

    def draw(self, plan, boxes):
        """``boxes``: float32 [n, 4] in canvas coordinates (already shifted by the expand)"""
        h, w = plan.canvas_hw
        while True:                                # quirk: no exit but a mode of 1 or an accepted patch, as the reference
            mode = random.choice(self.sample_mode)
            if mode == 1:
                return
            min_iou = mode
            for _ in range(50):
                new_w = random.uniform(self.min_crop_size * w, w)
                new_h = random.uniform(self.min_crop_size * h, h)
                if new_h / new_w < 0.5 or new_h / new_w > 2:
                    continue
                # quirk: the reference writes random.uniform(w - new_w), which is uniform(low=w - new_w, high=1.0)
                left = random.uniform(w - new_w)
                top = random.uniform(h - new_h)
                patch = np.array((int(left), int(top), int(left + new_w), int(top + new_h)))
                overlaps = bbox_overlaps(patch.reshape(-1, 4), boxes.reshape(-1, 4)).reshape(-1)
                if overlaps.min() < min_iou:
                    continue
                center = (boxes[:, :2] + boxes[:, 2:]) / 2
                mask = ((center[:, 0] > patch[0]) * (center[:, 1] > patch[1]) * (center[:, 0] < patch[2])
                        * (center[:, 1] < patch[3]))
                if not mask.any():
                    continue
                # (left + new_w < w + 1 and left >= 0 whichever way the quirk's bounds fall, so the patch stays on the canvas
                # and the reference's slice has the patch's size)
                assert 0 <= patch[0] < patch[2] <= w and 0 <= patch[1] < patch[3] <= h, (patch, h, w)
                plan.patch = tuple(int(v) for v in patch)
                plan.keep = mask.astype(bool)
                return


class ExtraAugmentation(object):
    """the reference's constructor keywords and defaults; ``draw`` instead of ``__call__`` (no pixels here)"""

    def __init__(self, photo_metric_distortion=None, expand=None, random_crop=None):
        self.photo_metric_distortion = (None if photo_metric_distortion is None
                                        else PhotoMetricDistortion(**photo_metric_distortion))
        self.expand = None if expand is None else Expand(**expand)
        self.random_crop = None if random_crop is None else RandomCrop(**random_crop)

    def draw(self, h, w, boxes, labels):
        """the reference's draws for an h x w image with these boxes -> ``AugPlan`` (``boxes`` / ``labels`` are not modified)"""
        boxes = np.array(boxes, dtype=np.float32).reshape(-1, 4)
        assert len(labels) == len(boxes)
        plan = AugPlan(h, w, len(boxes))
        if self.photo_metric_distortion is not None:
            self.photo_metric_distortion.draw(plan)
        if self.expand is not None:
            self.expand.draw(plan)
        if self.random_crop is not None:
            self.random_crop.draw(plan, boxes + np.tile((plan.left, plan.top), 2).astype(np.float32))
        return plan
