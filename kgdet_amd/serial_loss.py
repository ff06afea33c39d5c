"""Target assignment + the five loss families of the serial / parallel heads as five HIP launches (csrc/serial_loss.hip).

``RepPointsHeadKpSerial.loss`` / ``RepPointsHeadKpParallel.loss`` (reppoints_head_kp_serial.py loss / loss_single) assign the
init stage with ``PointAssigner`` and the refine stage with ``MaxIoUAssigner`` on the boxes of the init reppoints, build the
per-point targets of five pyramid levels with ``point_target_kp`` and evaluate five losses per level on decoded coordinates.
``kgdet_amd.heads_serial`` keeps that path (``points.point_target_kp_dense``, ``losses``) as chains of small torch ops.  For the
configuration config 5 trains -- PointAssigner with a fixed ``pos_num``, MaxIoUAssigner with ``gt_max_assign_all`` and no ignore
regions, sigmoid focal + smooth-L1 losses with ``reduction='mean'`` -- this module computes the same 5 x L numbers and the
gradients of the 5 x L maps from the raw prediction maps, the two box maps of ``moment.moment_bbox`` and the ground-truth
tables, without materialising a target or weight tensor and without a host read.

``KGDET_FUSED_SERIAL_LOSS=0`` selects the torch chain (A/B, and what the parity tests compare against).  The ``autograd.Function``
skeleton, the ground-truth pointers and the ground-truth check are ``head_loss.py``'s.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from .head_loss import MAX_IMAGES, FusedLoss, bind, fill_ground_truth, gt_why_not

ENABLED = os.environ.get('KGDET_FUSED_SERIAL_LOSS', '1') == '1'
MAX_LEVELS, MAX_LEVEL_POINTS, MAX_POS_NUM = 8, 32768, 64
FAMILIES = ('cls', 'box_init', 'box_refine', 'kpt_init', 'kpt_refine')                 # the order of kgdet_serial_maps
NAMES = ('loss_cls', 'loss_bbox_init', 'loss_bbox_refine', 'loss_kpt_init', 'loss_kpt_refine')


class SerialTargets(ctypes.Structure):
    _fields_ = [('B', ctypes.c_int32), ('L', ctypes.c_int32), ('num_classes', ctypes.c_int32), ('num_keypoints', ctypes.c_int32),
                ('H', ctypes.c_int32 * MAX_LEVELS), ('W', ctypes.c_int32 * MAX_LEVELS), ('stride', ctypes.c_float * MAX_LEVELS),
                ('num_gt', ctypes.c_int32 * MAX_IMAGES), ('gt_bboxes', ctypes.c_void_p * MAX_IMAGES),
                ('gt_labels', ctypes.c_void_p * MAX_IMAGES), ('gt_keypoints', ctypes.c_void_p * MAX_IMAGES),
                ('valid_h', (ctypes.c_int32 * MAX_LEVELS) * MAX_IMAGES), ('valid_w', (ctypes.c_int32 * MAX_LEVELS) * MAX_IMAGES)]


class SerialLossCfg(ctypes.Structure):
    _fields_ = [('pos_num', ctypes.c_int32), ('scale', ctypes.c_float), ('pos_iou_thr', ctypes.c_float),
                ('neg_lo', ctypes.c_float), ('neg_hi', ctypes.c_float), ('min_pos_iou', ctypes.c_float),
                ('pos_weight', ctypes.c_float), ('point_base_scale', ctypes.c_float), ('gamma', ctypes.c_float),
                ('alpha', ctypes.c_float), ('beta', ctypes.c_float * 4), ('loss_weight', ctypes.c_float * 5)]


class SerialMaps(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p * MAX_LEVELS) for n in FAMILIES]


def _maps(tensors, L):
    """``tensors``: family-major, level-minor (5 x L)"""
    m = SerialMaps()
    for f, name in enumerate(FAMILIES):
        for l in range(L):
            getattr(m, name)[l] = tensors[f * L + l].data_ptr()
    return m


def valid_sizes(head, img_metas, featmap_sizes):
    """per image and level the (rows, columns) of the grid inside its pad_shape (get_points' valid flags)"""
    return [[(min(int(np.ceil(meta['pad_shape'][0] / s)), fs[0]), min(int(np.ceil(meta['pad_shape'][1] / s)), fs[1]))
             for s, fs in zip(head.point_strides, featmap_sizes)] for meta in img_metas]


def _assigners(cfg):
    return cfg.init.assigner, cfg.refine.assigner


def applicable(head, cfg, cls_scores, keypts_preds_init, keypts_preds_refine, reppts_preds_init, reppts_preds_refine,
               gt_bboxes, gt_labels, gt_keypoints, img_metas, gt_bboxes_ignore=None):
    """the fused kernels cover exactly: float32 CUDA maps outside autocast; focal + four smooth-L1 losses with 'mean';
    PointAssigner with a fixed pos_num for the init stage; MaxIoUAssigner with gt_max_assign_all and without ignore regions
    for the refine stage; consecutive power-of-two strides; ground truth on the maps' device within the header's limits"""
    return why_not(head, cfg, cls_scores, keypts_preds_init, keypts_preds_refine, reppts_preds_init, reppts_preds_refine,
                   gt_bboxes, gt_labels, gt_keypoints, img_metas, gt_bboxes_ignore) is None


def why_not(head, cfg, cls_scores, keypts_preds_init, keypts_preds_refine, reppts_preds_init, reppts_preds_refine,
            gt_bboxes, gt_labels, gt_keypoints, img_metas, gt_bboxes_ignore=None):
    """None when ``applicable``, else the reason in words"""
    from .losses import FocalLoss, SmoothL1Loss
    if not ENABLED:
        return 'the fused serial loss is switched off (KGDET_FUSED_SERIAL_LOSS=0)'
    if head.sampling or not head.use_sigmoid_cls:
        return 'the head samples or has a softmax classifier'
    if type(head.loss_cls) is not FocalLoss or head.loss_cls.reduction != 'mean':
        return 'loss_cls is not FocalLoss with reduction "mean"'
    for n in NAMES[1:]:
        m = getattr(head, n)
        if type(m) is not SmoothL1Loss or m.reduction != 'mean' or not m.beta > 0:
            return '%s is not SmoothL1Loss with reduction "mean" and a positive beta' % n
    if not (gt_bboxes_ignore is None or all(g is None for g in gt_bboxes_ignore)):
        return 'the batch carries gt_bboxes_ignore'
    ai, ar = _assigners(cfg)
    if ai.get('type') != 'PointAssigner' or ai.get('pos_scale_factor') is not None:
        return 'the init assigner is no PointAssigner with a fixed pos_num'
    if ar.get('type') != 'MaxIoUAssigner' or not ar.get('gt_max_assign_all', True) or not ar.get('ignore_iof_thr', -1) < 0:
        return 'the refine assigner is no MaxIoUAssigner with gt_max_assign_all and without ignore regions'
    neg = ar.get('neg_iou_thr')
    if not (isinstance(neg, float) or (isinstance(neg, (tuple, list)) and len(neg) == 2)):
        return 'neg_iou_thr is neither a float nor a pair'
    strides = list(head.point_strides)
    L = len(strides)
    if not 1 <= L <= MAX_LEVELS or len(cls_scores) != L:
        return 'not 1..%d pyramid levels, one map each' % MAX_LEVELS
    first = strides[0]
    if first < 1 or int(first) != first or int(first) & (int(first) - 1) or \
            any(strides[l] != 2 * strides[l - 1] for l in range(1, L)):
        return 'the strides are not consecutive powers of two'
    t0 = cls_scores[0]
    B = t0.shape[0]
    if not t0.is_cuda or B > MAX_IMAGES or torch.is_autocast_enabled():
        return 'maps off the GPU, more than %d images, or autocast' % MAX_IMAGES
    for group in (cls_scores, keypts_preds_init, keypts_preds_refine, reppts_preds_init, reppts_preds_refine):
        if len(group) != L or any(m.dtype != torch.float32 or m.device != t0.device for m in group):
            return 'a family without one float32 map per level on one device'
    sizes = [tuple(m.shape[-2:]) for m in cls_scores]
    if any(h * w > MAX_LEVEL_POINTS for h, w in sizes):
        return 'a level of more than %d points' % MAX_LEVEL_POINTS
    pos_num = ai.get('pos_num', 3)
    if not 1 <= pos_num <= MAX_POS_NUM:
        return 'pos_num %d outside 1..%d' % (pos_num, MAX_POS_NUM)
    if any(vh * vw < pos_num for per in valid_sizes(head, img_metas, sizes) for vh, vw in per):
        return 'an image with fewer valid points than pos_num on some level'
    if len(gt_bboxes) != B:
        return 'not one ground-truth tensor per image'
    if any(k.shape[0] != g.shape[0] for g, k in zip(gt_bboxes, gt_keypoints)):
        return 'an image whose keypoints and boxes differ in number'
    return gt_why_not(B, t0.device, head.num_keypts, gt_bboxes, gt_labels, gt_keypoints)


def descriptors(head, cfg, featmap_sizes, sizes_valid, gt_bboxes, gt_labels, gt_keypoints):
    """(kgdet_serial_targets, kgdet_serial_loss_cfg, the contiguous ground-truth tensors the pointers refer to)"""
    B, L = len(gt_bboxes), len(featmap_sizes)
    t = SerialTargets()
    t.B, t.L, t.num_classes, t.num_keypoints = B, L, head.cls_out_channels, head.num_keypts
    for l, (h, w) in enumerate(featmap_sizes):
        t.H[l], t.W[l], t.stride[l] = int(h), int(w), float(head.point_strides[l])
    keep = fill_ground_truth(t, gt_bboxes, gt_labels, gt_keypoints)
    for b in range(B):
        for l in range(L):
            t.valid_h[b][l], t.valid_w[b][l] = int(sizes_valid[b][l][0]), int(sizes_valid[b][l][1])
    ai, ar = _assigners(cfg)
    c = SerialLossCfg()
    c.pos_num, c.scale = int(ai.get('pos_num', 3)), float(ai.get('scale', 4))
    neg = ar['neg_iou_thr']
    c.pos_iou_thr, c.min_pos_iou = float(ar['pos_iou_thr']), float(ar.get('min_pos_iou', .0))
    c.neg_lo, c.neg_hi = (0.0, float(neg)) if isinstance(neg, float) else (float(neg[0]), float(neg[1]))
    c.pos_weight = 1.0 if cfg.refine.pos_weight <= 0 else float(cfg.refine.pos_weight)
    c.point_base_scale = float(head.point_base_scale)
    c.gamma, c.alpha = float(head.loss_cls.gamma), float(head.loss_cls.alpha)
    c.loss_weight[0] = float(head.loss_cls.loss_weight)
    for k, n in enumerate(NAMES[1:]):
        c.beta[k], c.loss_weight[1 + k] = float(getattr(head, n).beta), float(getattr(head, n).loss_weight)
    return t, c, keep


def inputs(head, cfg, cls_scores, keypts_preds_init, keypts_preds_refine, reppts_preds_init, reppts_preds_refine,
           gt_bboxes, gt_labels, gt_keypoints, img_metas):
    """(targets, cfg, kept ground truth, the 5 x L maps family-major) of one call"""
    sizes = [tuple(m.shape[-2:]) for m in cls_scores]
    t, c, keep = descriptors(head, cfg, sizes, valid_sizes(head, img_metas, sizes), gt_bboxes, gt_labels, gt_keypoints)
    # the head's points2bbox of the raw reppoints, stride units: ONE moment box per stage and level (the torch chain evaluates
    # the init box twice: detached for the refine assigner, and for the loss)
    box_init = [head.points2bbox(r) for r in reppts_preds_init]
    box_refine = [head.points2bbox(r) for r in reppts_preds_refine]
    return t, c, keep, list(cls_scores) + box_init + box_refine + list(keypts_preds_init) + list(keypts_preds_refine)


def serial_loss(head, cfg, *args):
    """The five loss lists of ``head.loss`` (one 0-dim tensor per level, as the reference returns); arguments as ``inputs``."""
    t, c, keep, maps = inputs(head, cfg, *args)
    L = t.L
    lib = _lib.lib()
    out = FusedLoss.apply(bind(lib.kgdet_serial_loss_forward, t, c), bind(lib.kgdet_serial_loss_backward, t, c),
                          lib.kgdet_serial_loss_workspace_bytes(ctypes.byref(t), ctypes.byref(c)), 5 * L,
                          lambda tensors: _maps(tensors, L), keep, *maps)
    return {n: list(out[k * L:(k + 1) * L]) for k, n in enumerate(NAMES)}
