"""Target assignment + the nine losses of the KGDet head as four HIP launches (csrc/head_loss.hip).

``RepPointsHeadKp3RepCas1AssignOnce.loss`` (reppoints_head_kp3rep_cas_1_assign_once.py:581-665) builds its targets with
``PointAssigner`` / ``point_target_kp`` and evaluates 3 x (FocalLoss, SmoothL1Loss boxes, SmoothL1Loss keypoints) on
decoded coordinates.  ``kgdet_amd.heads`` keeps that path, expression by expression (``points.point_target_kp_dense``,
``losses``): ~650 small torch launches per step.  For the configuration the KGDet configs train -- one pyramid level, all
points valid, PointAssigner with a fixed ``pos_num``, sigmoid focal + smooth-L1 losses with ``reduction='mean'`` -- this
module computes the same nine numbers and the same nine gradients from the raw prediction maps and the ground-truth
tables, without materialising a target or weight tensor and without a host read.

``KGDET_FUSED_HEAD_LOSS=0`` selects the torch chain (A/B, and what the parity tests compare against).

What the wrapper of the serial / parallel heads' fused loss (``serial_loss.py``) needs as well lives here once: the ground-truth
check, the ground-truth pointers of a targets descriptor, and the ``autograd.Function`` around a forward / backward call pair.

The table route (``gt_table`` / ``gt_capacity``): the per-image ground-truth counts and valid extents are read from a device
table [B, 4] int32 = (num_gt, valid_h, valid_w, 0) when the kernels run, and every ground-truth tensor is a buffer of
``gt_capacity`` rows of which the first ``num_gt`` count -- the launch arguments no longer depend on the batch
(``static_batch.StaticBatch`` holds such buffers).  The padded rows exist for the kernels alone: with a table there is no torch chain to fall to, ``why_not`` names what stands in the way.
"""
import ctypes
import os

import torch

from . import _lib

ENABLED = os.environ.get('KGDET_FUSED_HEAD_LOSS', '1') == '1'
MAX_IMAGES, MAX_GT, MAX_POINTS = 16, 64, 4096            # MAX_IMAGES, MAX_GT: both loss families' (csrc/loss_math.h)


class HeadTargets(ctypes.Structure):
    _fields_ = [('B', ctypes.c_int32), ('H', ctypes.c_int32), ('W', ctypes.c_int32), ('num_classes', ctypes.c_int32),
                ('num_keypoints', ctypes.c_int32), ('stride', ctypes.c_float),
                ('num_gt', ctypes.c_int32 * MAX_IMAGES), ('gt_bboxes', ctypes.c_void_p * MAX_IMAGES),
                ('gt_labels', ctypes.c_void_p * MAX_IMAGES), ('gt_keypoints', ctypes.c_void_p * MAX_IMAGES),
                ('valid_h', ctypes.c_int32 * MAX_IMAGES), ('valid_w', ctypes.c_int32 * MAX_IMAGES)]


class HeadLossCfg(ctypes.Structure):
    _fields_ = [('pos_num', ctypes.c_int32), ('pos_weight', ctypes.c_float), ('normalize_term', ctypes.c_float),
                ('gamma', ctypes.c_float * 3), ('alpha', ctypes.c_float * 3), ('beta', ctypes.c_float * 6),
                ('loss_weight', ctypes.c_float * 9)]


class HeadMaps(ctypes.Structure):
    _fields_ = [('cls', ctypes.c_void_p * 3), ('bbox', ctypes.c_void_p * 3), ('kpt', ctypes.c_void_p * 3)]


def _maps(tensors):
    m = HeadMaps()
    for s in range(3):
        m.cls[s], m.bbox[s], m.kpt[s] = tensors[s].data_ptr(), tensors[3 + s].data_ptr(), tensors[6 + s].data_ptr()
    return m


# ---- shared with serial_loss.py: the ground-truth check, the ground-truth pointers, the autograd.Function of a call pair
def gt_why_not(B, device, num_keypts, gt_bboxes, gt_labels, gt_keypoints, cap=None):
    """None when the kernels can take the ground truth of ``B`` images for maps on ``device``, else the reason in words.
    ``cap``: the table route -- every tensor is a buffer of at least ``cap`` rows, and the counts are not the host's to check."""
    for b in range(B):
        g = gt_bboxes[b].shape[0]
        if cap is not None:
            if g < cap or gt_keypoints[b].shape[0] < cap or gt_labels[b].shape[0] < cap:
                return 'image %d: a ground-truth buffer is shorter than the capacity of %d rows' % (b, cap)
        elif g < 1 or g > MAX_GT:
            return 'image %d: %d ground truths (1..%d)' % (b, g, MAX_GT)
        if gt_bboxes[b].dtype != torch.float32 or gt_keypoints[b].dtype != torch.float32 or \
                gt_keypoints[b].shape[1:] != (num_keypts, 3):
            return 'image %d: ground truth that is not float32 [n, 4] and [n, %d, 3]' % (b, num_keypts)
        # the kernels dereference the raw ground-truth pointers: they must live on the maps' device (CPU-resident or
        # other-GPU ground truth takes the torch chain, which raises torch's own device-mismatch error or works)
        if gt_bboxes[b].device != device or gt_keypoints[b].device != device:
            return 'image %d: ground truth on another device than the maps' % b
        if gt_labels is not None and gt_labels[b] is not None and (gt_labels[b].dtype != torch.int64 or
                                                                   gt_labels[b].device != device):
            return 'image %d: labels that are not int64 on the maps\' device' % b
    return None


def fill_ground_truth(t, gt_bboxes, gt_labels, gt_keypoints, counts=True):
    """the ground-truth pointers of the ``t.B`` images (with ``counts``: and ``num_gt``) of a targets descriptor; returns the
    contiguous tensors the pointers refer to, which must outlive the calls"""
    keep = []
    for b in range(t.B):
        bb, kp = gt_bboxes[b].contiguous(), gt_keypoints[b].contiguous()
        if bb.shape[0] == 0:
            raise ValueError('No gt or bboxes')
        lab = None if gt_labels is None or gt_labels[b] is None else gt_labels[b].contiguous()
        keep += [bb, kp, lab]
        if counts:
            t.num_gt[b] = bb.shape[0]
        t.gt_bboxes[b], t.gt_keypoints[b] = bb.data_ptr(), kp.data_ptr()
        t.gt_labels[b] = lab.data_ptr() if lab is not None else None
    return keep


def bind(fn, targets, cfg, *extra):
    """a library call of either family as ``call(maps descriptor, *rest)``: fn(targets, cfg, maps, *extra, *rest), status checked"""
    def call(hm, *rest):
        _lib.check(fn(ctypes.byref(targets), ctypes.byref(cfg), ctypes.byref(hm), *extra, *rest), fn.__name__)
    return call


class FusedLoss(torch.autograd.Function):
    """``apply(forward, backward, ws_bytes, n, describe, keep, *maps)`` -> ``n`` 0-dim losses.  ``forward`` / ``backward``: the two
    library calls (``bind``); ``describe``: tensors -> maps descriptor; ``keep``: whatever the descriptors point at."""

    @staticmethod
    def forward(ctx, forward, backward, ws_bytes, n, describe, keep, *maps):
        maps = tuple(m.contiguous() for m in maps)
        dev = maps[0].device
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        # the losses, then num_total: two floats for the serial heads, one (and an unused slot) for the KGDet head
        out = torch.empty(n + 2, dtype=torch.float32, device=dev)
        forward(describe(maps), _lib.ptr(out), ctypes.c_void_p(out.data_ptr() + 4 * n), _lib.ptr(ws), ctypes.c_size_t(ws_bytes),
                _lib.current_stream())
        ctx.call = (backward, ws_bytes, n, describe, keep, ws, out)
        ctx.save_for_backward(*maps)
        return tuple(out[k] for k in range(n))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grad_losses):
        maps = ctx.saved_tensors
        backward, ws_bytes, n, describe, _, ws, out = ctx.call
        zero = torch.zeros((), dtype=torch.float32, device=maps[0].device) if any(g is None for g in grad_losses) else None
        up = torch.stack([(zero if g is None else g).reshape(()).float() for g in grad_losses])
        grads = tuple(torch.empty_like(m) for m in maps)
        hg = describe(grads)
        backward(describe(maps), _lib.ptr(up), ctypes.c_void_p(out.data_ptr() + 4 * n), ctypes.byref(hg), _lib.ptr(ws),
                 ctypes.c_size_t(ws_bytes), _lib.current_stream())
        return (None,) * 6 + grads


# ---- the KGDet head
def applicable(head, cfg, cls_scores, kpt_preds, bbox_preds, gt_bboxes, gt_labels, gt_keypoints, gt_bboxes_ignore,
               all_valid=True, valid_sizes=None, gt_table=None, gt_capacity=None):
    """the fused kernels cover exactly the case ``points.dense_targets_applicable`` covers for one level, on the GPU, in
    float32; ``valid_sizes``: per image the (rows, columns) of the grid inside its pad_shape (None: all of it).
    ``gt_table`` (a device table of counts and extents, see the module's docstring): the ground-truth tensors are buffers of
    ``gt_capacity`` rows -- the per-image count checks become checks of the capacity, the extents are the table's."""
    return why_not(head, cfg, cls_scores, kpt_preds, bbox_preds, gt_bboxes, gt_labels, gt_keypoints, gt_bboxes_ignore,
                   all_valid, valid_sizes, gt_table, gt_capacity) is None


def table_capacity(gt_bboxes, gt_capacity=None):
    """the row capacity of the table route's ground-truth buffers: ``gt_capacity``, or the buffers' own length"""
    return int(gt_bboxes[0].shape[0]) if gt_capacity is None else int(gt_capacity)


def why_not(head, cfg, cls_scores, kpt_preds, bbox_preds, gt_bboxes, gt_labels, gt_keypoints, gt_bboxes_ignore,
            all_valid=True, valid_sizes=None, gt_table=None, gt_capacity=None):
    """None when ``applicable``, else the reason in words"""
    from .losses import FocalLoss, SmoothL1Loss
    from .points import dense_targets_applicable
    if not ENABLED:
        return 'the fused head loss is switched off (KGDET_FUSED_HEAD_LOSS=0)'
    if head.sampling or not head.use_sigmoid_cls or len(head.point_strides) != 1:
        return 'the head samples, has a softmax classifier or more than one pyramid level'
    if not dense_targets_applicable(cfg, 1, all_valid, gt_bboxes_ignore):
        return 'the assigner is no PointAssigner with a fixed pos_num, or the batch carries gt_bboxes_ignore'
    for stage in (1, 2, 3):
        lc, lb, lk = (getattr(head, 'loss_%s_%d' % (n, stage)) for n in ('cls', 'bbox', 'kpt'))
        if type(lc) is not FocalLoss or lc.reduction != 'mean' or type(lb) is not SmoothL1Loss or \
                type(lk) is not SmoothL1Loss or lb.reduction != 'mean' or lk.reduction != 'mean':
            return 'stage %d: the losses are not FocalLoss / SmoothL1Loss with reduction "mean"' % stage
    t0 = cls_scores[0][0]
    B, _, H, W = t0.shape
    if not t0.is_cuda or B > MAX_IMAGES or H * W > MAX_POINTS or torch.is_autocast_enabled():
        return 'maps off the GPU, more than %d images, more than %d points, or autocast' % (MAX_IMAGES, MAX_POINTS)
    for group in (cls_scores, kpt_preds, bbox_preds):
        for per_level in group:
            if len(per_level) != 1 or per_level[0].dtype != torch.float32:
                return 'more than one level, or maps that are not float32'
    if cfg.assigner.get('pos_num', 3) > H * W:
        return 'pos_num beyond the number of points'
    if valid_sizes is not None and any(vh * vw < cfg.assigner.get('pos_num', 3) for vh, vw in valid_sizes):
        return 'an image with fewer valid points than pos_num'
    cap = None
    if gt_table is not None:
        cap = table_capacity(gt_bboxes, gt_capacity)
        if not 1 <= cap <= MAX_GT:
            return 'gt_capacity %d outside 1..%d' % (cap, MAX_GT)
        if gt_table.dtype != torch.int32 or tuple(gt_table.shape) != (B, 4) or gt_table.device != t0.device or \
                not gt_table.is_contiguous():
            return 'the table is not a contiguous int32 [%d, 4] tensor on the maps\' device' % B
        if gt_labels is None or any(l is None for l in gt_labels):
            return 'the table route needs label buffers'
    return gt_why_not(B, t0.device, head.num_keypts, gt_bboxes, gt_labels, gt_keypoints, cap)


def head_loss(head, cfg, cls_scores, kpt_preds, bbox_preds, gt_bboxes, gt_labels, gt_keypoints, valid_sizes=None,
              gt_table=None, gt_capacity=None):
    """The nine losses of ``head.loss`` as a dict of 0-dim tensors (one list entry per level, as the reference returns).
    ``cls_scores`` / ``kpt_preds`` / ``bbox_preds``: three stages x [one level] of NCHW maps.  ``gt_table``: the table route
    (the module's docstring) -- counts and extents are the table's, ``valid_sizes`` is not used."""
    cap = None if gt_table is None else table_capacity(gt_bboxes, gt_capacity)
    t0 = cls_scores[0][0]
    B, C, H, W = t0.shape
    t = HeadTargets()
    t.B, t.H, t.W, t.num_classes, t.num_keypoints = B, H, W, C, head.num_keypts
    t.stride = float(head.point_strides[0])
    keep = fill_ground_truth(t, gt_bboxes, gt_labels, gt_keypoints, counts=gt_table is None)
    if valid_sizes is not None and gt_table is None:
        for b in range(B):
            t.valid_h[b], t.valid_w[b] = int(valid_sizes[b][0]), int(valid_sizes[b][1])
    c = HeadLossCfg()
    a = cfg.assigner
    c.pos_num = int(a.get('pos_num', 3))
    c.pos_weight = 1.0 if cfg.pos_weight <= 0 else float(cfg.pos_weight)
    c.normalize_term = float(head.point_base_scale * head.point_strides[0])
    for s in range(3):
        lc, lb, lk = (getattr(head, 'loss_%s_%d' % (n, s + 1)) for n in ('cls', 'bbox', 'kpt'))
        c.gamma[s], c.alpha[s] = float(lc.gamma), float(lc.alpha)
        c.beta[s], c.beta[3 + s] = float(lb.beta), float(lk.beta)
        c.loss_weight[s], c.loss_weight[3 + s], c.loss_weight[6 + s] = float(lc.loss_weight), float(lb.loss_weight), \
            float(lk.loss_weight)
    maps = [cls_scores[s][0] for s in range(3)] + [bbox_preds[s][0] for s in range(3)] + [kpt_preds[s][0] for s in range(3)]
    L = _lib.lib()
    if gt_table is None:
        calls = bind(L.kgdet_head_loss_forward, t, c), bind(L.kgdet_head_loss_backward, t, c)
    else:
        table = (_lib.ptr(gt_table), ctypes.c_int32(cap))
        calls = bind(L.kgdet_head_loss_forward_table, t, c, *table), bind(L.kgdet_head_loss_backward_table, t, c, *table)
    out = FusedLoss.apply(*calls, L.kgdet_head_loss_workspace_bytes(ctypes.byref(t)), 9, _maps, (keep, gt_table), *maps)
    names = ['loss_cls_1', 'loss_cls_2', 'loss_cls_3', 'loss_bbox_1', 'loss_bbox_2', 'loss_bbox_3',
             'loss_kpt_1', 'loss_kpt_2', 'loss_kpt_3']
    return {n: [v] for n, v in zip(names, out)}
