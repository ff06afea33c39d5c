"""Two-stage (init -> refine) keypoint RepPoints heads over the whole FPN pyramid:
``RepPointsHeadKpSerial`` and ``RepPointsHeadKpParallel`` (BASELINE config 5).

Host-side mirror of mmdet/models/anchor_heads/reppoints_head_kp_serial.py:16-750 (SER) and
reppoints_head_kp_parallel.py (identical except that the reppoints get their own conv /
deformable-conv branch instead of being regressed from the keypoints, :153-168, 314-315, 331-332).
Same registered names, constructor arguments and parameter names.  Per level one 3x3 deformable
conv for classification and one for keypoints (plus one for reppoints in the parallel head), all
through the HIP kernel; the init stage is assigned by ``PointAssigner``, the refine stage by
``MaxIoUAssigner`` on the boxes of the init reppoints (SER:551-573).

Reference quirks kept so that outputs stay identical: the decode step clamps ``kpts[:, 0::3]`` /
``kpts[:, 1::3]`` (the keypoint axis, SER:723-724) where the KGDet head clamps the coordinate axis;
keypoint weights are normalised per row without the x4 of the KGDet head (SER:469-477).
"""
from __future__ import division

import os

import numpy as np
import torch
import torch.nn as nn

from . import conv1x1, dcn, decode, serial_loss
from .heads import PointHeadMixin
from .layers import ConvModule, bias_init_with_prob, normal_init, shared_levels
from .losses import SmoothL1Loss
from .points import (PointGenerator, dense_targets_applicable, multi_apply, point_target_kp,
                     point_target_kp_dense)
from .registry import HEADS, build_loss

GROUPED_REFINE = os.environ.get('KGDET_SERIAL_GROUPED_DCN', '1') == '1'      # 0: one call per deformable convolution (A/B)
SHARED_LEVELS = os.environ.get('KGDET_SERIAL_SHARED_LEVELS', '1') == '1'     # 0: five autograd sub-graphs, engine-side gradient adds (A/B)
DENSE_TARGETS = os.environ.get('KGDET_SERIAL_DENSE_TARGETS', '1') == '1'     # 0: the reference-mirroring (host-syncing) path (A/B)


class _RepPointsHeadKpTwoStage(PointHeadMixin, nn.Module):
    parallel_reppts = False  # True: reppoints have their own conv branches (parallel head)

    def __init__(self,
                 num_classes,
                 in_channels,
                 feat_channels=256,
                 point_feat_channels=256,
                 stacked_convs=3,
                 num_reppts=9,
                 num_keypts=17,
                 gradient_mul=0.1,
                 point_strides=[8, 16, 32, 64, 128],
                 point_base_scale=4,
                 conv_cfg=None,
                 norm_cfg=None,
                 loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 loss_bbox_init=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=0.5),
                 loss_bbox_refine=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0),
                 loss_kpt_init=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=0.5),
                 loss_kpt_refine=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0),
                 use_grid_points=False,
                 center_init=True,
                 transform_method='moment',
                 moment_mul=0.01):
        super().__init__()
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.feat_channels = feat_channels
        self.point_feat_channels = point_feat_channels
        self.stacked_convs = stacked_convs
        self.num_keypts = num_keypts
        self.num_reppts = num_reppts
        self.gradient_mul = gradient_mul
        self.point_base_scale = point_base_scale
        self.point_strides = point_strides
        self.conv_cfg = conv_cfg
        self.norm_cfg = norm_cfg
        self.use_sigmoid_cls = loss_cls.get('use_sigmoid', False)
        self.sampling = loss_cls['type'] not in ['FocalLoss']
        self.loss_cls = build_loss(loss_cls)
        self.loss_bbox_init = build_loss(loss_bbox_init)
        self.loss_bbox_refine = build_loss(loss_bbox_refine)
        self.loss_kpt_init = build_loss(loss_kpt_init)
        self.loss_kpt_refine = build_loss(loss_kpt_refine)
        self.use_grid_points = use_grid_points
        self.center_init = center_init
        self.transform_method = transform_method
        if self.transform_method == 'moment':
            self.moment_transfer = nn.Parameter(data=torch.zeros(2), requires_grad=True)
            self.moment_mul = moment_mul
        self.cls_out_channels = self.num_classes - 1 if self.use_sigmoid_cls else self.num_classes
        self.point_generators = [PointGenerator() for _ in self.point_strides]
        # the reppoints are the taps of a sqrt(n) x sqrt(n) deformable conv
        self.dcn_kernel = int(np.sqrt(num_reppts))
        self.dcn_pad = int((self.dcn_kernel - 1) / 2)
        assert self.dcn_kernel * self.dcn_kernel == num_reppts, 'The points number should be a square number.'
        assert self.dcn_kernel % 2 == 1, 'The points number should be an odd square number.'
        base = np.arange(-self.dcn_pad, self.dcn_pad + 1).astype(np.float64)
        yx = np.stack([np.repeat(base, self.dcn_kernel), np.tile(base, self.dcn_kernel)], axis=1).reshape(-1)
        self.dcn_base_offset = torch.tensor(yx).view(1, -1, 1, 1)
        self._init_layers()

    def _init_layers(self):
        self.relu = nn.ReLU(inplace=False)
        self.cls_convs = nn.ModuleList()
        self.reg_convs = nn.ModuleList()
        for i in range(self.stacked_convs):
            chn = self.in_channels if i == 0 else self.feat_channels
            self.cls_convs.append(ConvModule(chn, self.feat_channels, 3, stride=1, padding=1,
                                             conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg))
            self.reg_convs.append(ConvModule(chn, self.feat_channels, 3, stride=1, padding=1,
                                             conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg))
        keypts_out_dim = 2 * self.num_keypts
        reppts_out_dim = 2 * self.num_reppts
        fc, pc, k, pad = self.feat_channels, self.point_feat_channels, self.dcn_kernel, self.dcn_pad
        self.cls_refine_dfmconv = dcn.DeformConv(fc, pc, k, 1, pad)
        self.cls_refine_out = nn.Conv2d(pc, self.cls_out_channels, 1, 1, 0)
        self.keypts_init_conv = nn.Conv2d(fc, pc, 3, 1, 1)
        self.keypts_init_out = nn.Conv2d(pc, keypts_out_dim, 1, 1, 0)
        if self.parallel_reppts:
            self.reppts_init_conv = nn.Conv2d(fc, pc, 3, 1, 1)
        self.reppts_init_out = nn.Conv2d(pc if self.parallel_reppts else keypts_out_dim, reppts_out_dim, 1, 1, 0)
        self.keypts_refine_dfmconv = dcn.DeformConv(fc, pc, k, 1, pad)
        self.keypts_refine_out = nn.Conv2d(pc, keypts_out_dim, 1, 1, 0)
        if self.parallel_reppts:
            self.reppts_refine_dfmconv = dcn.DeformConv(fc, pc, k, 1, pad)
        self.reppts_refine_out = nn.Conv2d(pc if self.parallel_reppts else keypts_out_dim, reppts_out_dim, 1, 1, 0)

    def init_weights(self):
        for m in self.cls_convs:
            normal_init(m.conv, std=0.01)
        for m in self.reg_convs:
            normal_init(m.conv, std=0.01)
        bias_cls = bias_init_with_prob(0.01)
        normal_init(self.cls_refine_dfmconv, std=0.01)
        normal_init(self.cls_refine_out, std=0.01, bias=bias_cls)
        normal_init(self.keypts_init_conv, std=0.01)
        normal_init(self.keypts_init_out, std=0.01)
        normal_init(self.reppts_init_out, std=0.01)
        normal_init(self.keypts_refine_dfmconv, std=0.01)
        normal_init(self.keypts_refine_out, std=0.01)
        normal_init(self.reppts_refine_out, std=0.01)
        if self.parallel_reppts:
            normal_init(self.reppts_init_conv, std=0.01)
            normal_init(self.reppts_refine_dfmconv, std=0.01)

    # KGDET_SERIAL_CL=1 (A/B, off): inference under autocast with the towers on the pyramid's channels-last maps as they come --
    # MIOpen's NHWC kernels without the layout conversions it wraps around NCHW calls (~100 launches, ~1 ms of a batch of 8).
    # Measured 402.8 against 424.0 img/s: GroupNorm on a channels-last map reads 16 bytes of every 512 (a group's 8 channels of
    # a pixel) -- gn_split_moments 150 us against 51 us at 100 x 168 -- and the deformable stages need an NCHW copy per tower.
    channels_last_inference = os.environ.get('KGDET_SERIAL_CL', '0') == '1'

    def _dfm(self, conv, feat, offset):
        """relu(deform_conv) with the ReLU fused into the kernel epilogue"""
        return dcn.deform_conv_cat(feat, [offset], [conv.weight], [self.dcn_pad])

    def forward_single(self, x):
        # (the reference keeps the regular grid as a plain CPU attribute and uploads it with type_as() on every call: a
        #  blocking host->device copy per level and step; uploaded once per device / dtype here)
        cache = self.__dict__.setdefault('_base_offset_cache', {})
        key = (x.device, x.dtype)
        if key not in cache:
            cache[key] = self.dcn_base_offset.to(device=x.device, dtype=x.dtype)
        dcn_base_offset = cache[key]
        if self.use_grid_points or not self.center_init:
            scale = self.point_base_scale / 2
            reppts_init = dcn_base_offset / dcn_base_offset.max() * scale
            keypts_init = 0
        else:
            reppts_init = 0
            keypts_init = 0
        cls_feat = x
        pts_feat = x
        for cls_conv in self.cls_convs:
            cls_feat = cls_conv(cls_feat)
        for reg_conv in self.reg_convs:
            pts_feat = reg_conv(pts_feat)
        # init stage
        # (the biased 3x3 convolutions + ReLU on the split-operand MFMA kernels, as in the KGDet head's first stage)
        keypts_out_init = conv1x1.conv_bias_act(self.keypts_init_out, conv1x1.conv_bias_act(self.keypts_init_conv, pts_feat, relu=True))
        if self.parallel_reppts:
            reppts_out_init = conv1x1.conv_bias_act(self.reppts_init_out, conv1x1.conv_bias_act(self.reppts_init_conv, pts_feat, relu=True))
        else:
            reppts_out_init = conv1x1.conv_bias_act(self.reppts_init_out, keypts_out_init)
        # (adding the integer 0 of the centre-init case would be a pass over a [B, 588, H, W] tensor for nothing)
        if not (isinstance(reppts_init, int) and reppts_init == 0):
            reppts_out_init = reppts_out_init + reppts_init
        if not (isinstance(keypts_init, int) and keypts_init == 0):
            keypts_out_init = keypts_out_init + keypts_init
        # refine stage: taps on the (gradient-scaled) init reppoints
        grad_mul = self.gradient_mul * reppts_out_init + (1 - self.gradient_mul) * reppts_out_init.detach()
        dcn_offset = grad_mul - dcn_base_offset
        # the refine stage's deformable convolutions share their offsets: ONE grouped call (one set of tap / inverse records,
        # grouped launches forward and backward, ReLU in the epilogue) instead of two or three
        if GROUPED_REFINE and cls_feat.is_cuda and not self.parallel_reppts:
            cls_dfm, kpt_dfm = dcn.deform_conv_cat_multi(
                [cls_feat, pts_feat], [dcn_offset],
                [[self.cls_refine_dfmconv.weight], [self.keypts_refine_dfmconv.weight]], [self.dcn_pad])
        else:
            cls_dfm = self._dfm(self.cls_refine_dfmconv, cls_feat, dcn_offset)
            kpt_dfm = self._dfm(self.keypts_refine_dfmconv, pts_feat, dcn_offset)
        cls_out = conv1x1.conv_bias_act(self.cls_refine_out, cls_dfm)
        keypts_out_refine = conv1x1.conv_bias_act(self.keypts_refine_out, kpt_dfm)
        if self.parallel_reppts:
            reppts_out_refine = conv1x1.conv_bias_act(self.reppts_refine_out, self._dfm(self.reppts_refine_dfmconv, pts_feat, dcn_offset))
        else:
            reppts_out_refine = conv1x1.conv_bias_act(self.reppts_refine_out, keypts_out_refine)
        keypts_out_refine = keypts_out_refine + keypts_out_init.detach()
        reppts_out_refine = reppts_out_refine + reppts_out_init.detach()
        return (cls_out, keypts_out_init, keypts_out_refine, reppts_out_init, reppts_out_refine)

    def forward(self, feats, img_metas):
        if SHARED_LEVELS and torch.is_grad_enabled() and feats[0].is_cuda and any(p.requires_grad for p in self.parameters()):
            # training: the five levels as ONE autograd node -- the shared parameters' gradients are summed over the levels by a few
            # multi-tensor launches inside it instead of 235 engine-side `add`s (layers.shared_levels)
            return shared_levels(self, self.forward_single, list(feats))
        return multi_apply(self.forward_single, feats)

    # ------------------------------------------------------------------------------------------
    def loss_single(self, cls_score, kpt_pred_init, kpt_pred_refine, rep_pred_init, rep_pred_refine, labels,
                    label_weights, bbox_gt_init, bbox_weights_init, bbox_gt_refine, bbox_weights_refine, kpt_gt_init,
                    kpt_weights_init, kpt_gt_refine, kpt_weights_refine, stride, num_total_samples_init,
                    num_total_samples_refine):
        labels = labels.reshape(-1)
        label_weights = label_weights.reshape(-1)
        cls_score = cls_score.permute(0, 2, 3, 1).reshape(-1, self.cls_out_channels)
        loss_cls = self.loss_cls(cls_score, labels, label_weights, avg_factor=num_total_samples_refine)

        normalize_term = self.point_base_scale * stride
        bbox_pred_init = self.points2bbox(rep_pred_init.reshape(-1, 2 * self.num_reppts), y_first=False)
        bbox_pred_refine = self.points2bbox(rep_pred_refine.reshape(-1, 2 * self.num_reppts), y_first=False)
        # (SmoothL1Loss takes the normalisation as `divisor`: the fused op reads the raw tensors -- no pred / d, target / d
        #  passes over [points, 588] tensors; same values)
        def normalised(loss_fn, pred, gt, weights, avg):
            if isinstance(loss_fn, SmoothL1Loss):
                return loss_fn(pred, gt, weights, avg_factor=avg, divisor=normalize_term)
            return loss_fn(pred / normalize_term, gt / normalize_term, weights, avg_factor=avg)

        loss_bbox_init = normalised(self.loss_bbox_init, bbox_pred_init, bbox_gt_init.reshape(-1, 4),
                                    bbox_weights_init.reshape(-1, 4), num_total_samples_init)
        loss_bbox_refine = normalised(self.loss_bbox_refine, bbox_pred_refine, bbox_gt_refine.reshape(-1, 4),
                                      bbox_weights_refine.reshape(-1, 4), num_total_samples_refine)

        def kpt_loss(loss_fn, pred, gt, weights, avg):
            # SER:469-477 normalises in place; with one image per GPU the per-level targets are views of one
            # tensor and the in-place update would invalidate weights autograd saved for another level, so
            # the normalisation runs on a private copy (same values)
            # (rows without a visible keypoint are all zero: dividing them by 1 gives the same tensor as the reference's
            #  boolean-mask update, without its device->host round trip)
            weights = weights.reshape(-1, self.num_keypts * 2)
            weights = weights / weights.sum(1).clamp(min=1).unsqueeze(1)
            return normalised(loss_fn, pred.reshape(-1, self.num_keypts * 2), gt.reshape(-1, self.num_keypts * 2), weights, avg)

        loss_kpt_init = kpt_loss(self.loss_kpt_init, kpt_pred_init, kpt_gt_init, kpt_weights_init,
                                 num_total_samples_init)
        loss_kpt_refine = kpt_loss(self.loss_kpt_refine, kpt_pred_refine, kpt_gt_refine, kpt_weights_refine,
                                   num_total_samples_refine)
        return loss_cls, loss_bbox_init, loss_bbox_refine, loss_kpt_init, loss_kpt_refine

    def loss(self, cls_scores, keypts_preds_init, keypts_preds_refine, reppts_preds_init, reppts_preds_refine,
             gt_bboxes, gt_labels, gt_keypoints, img_metas, cfg, gt_bboxes_ignore=None):
        featmap_sizes = [featmap.size()[-2:] for featmap in cls_scores]
        assert len(featmap_sizes) == len(self.point_generators)
        # both assignments, the decode and the five losses of every level as five HIP launches (csrc/serial_loss.hip) where the
        # configuration is the one config 5 trains; anything else takes the torch chain below (KGDET_FUSED_SERIAL_LOSS=0: always)
        maps = (cls_scores, keypts_preds_init, keypts_preds_refine, reppts_preds_init, reppts_preds_refine)
        if serial_loss.applicable(self, cfg, *maps, gt_bboxes, gt_labels, gt_keypoints, img_metas, gt_bboxes_ignore):
            return serial_loss.serial_loss(self, cfg, *maps, gt_bboxes, gt_labels, gt_keypoints, img_metas)
        label_channels = self.cls_out_channels if self.use_sigmoid_cls else 1
        device = cls_scores[0].device

        # init stage targets
        center_list, valid_flag_list = self.get_points(featmap_sizes, img_metas, device=device)
        kpt_coord_init = self.offset_to_pts(center_list, keypts_preds_init)
        rep_coord_init = self.offset_to_pts(center_list, reppts_preds_init)
        if cfg.init.assigner['type'] == 'PointAssigner':
            candidate_list = center_list
        else:
            candidate_list = self.centers_to_bboxes(center_list)
        # every grid point valid?  (host arithmetic on the image metas; if not, the dense path takes the valid flags)
        all_valid = all(
            min(int(np.ceil(meta['pad_shape'][0] / s)), fs[0]) == fs[0] and
            min(int(np.ceil(meta['pad_shape'][1] / s)), fs[1]) == fs[1]
            for meta in img_metas for s, fs in zip(self.point_strides, featmap_sizes))
        dense_ok = lambda c: (not self.sampling and DENSE_TARGETS and
                              dense_targets_applicable(c, len(self.point_strides), all_valid, gt_bboxes_ignore))
        if dense_ok(cfg.init):
            targets_init = point_target_kp_dense(candidate_list, gt_bboxes, gt_keypoints, cfg.init, gt_labels_list=gt_labels,
                                                 valid_flag_list=None if all_valid else valid_flag_list)
        else:
            targets_init = point_target_kp(candidate_list, valid_flag_list, gt_bboxes, gt_keypoints, img_metas, cfg.init,
                                           gt_bboxes_ignore_list=gt_bboxes_ignore, gt_labels_list=gt_labels,
                                           label_channels=label_channels, sampling=self.sampling)
        (*_, bbox_gt_list_init, candidate_list_init, bbox_weights_list_init, keypoint_gt_list_init,
         keypoint_weights_list_init, num_total_pos_init, num_total_neg_init) = targets_init
        num_total_samples_init = (num_total_pos_init + num_total_neg_init if self.sampling else num_total_pos_init)

        # refine stage targets: boxes of the (detached) init reppoints, MaxIoUAssigner
        center_list, valid_flag_list = self.get_points(featmap_sizes, img_metas, device=device)
        kpt_coord_refine = self.offset_to_pts(center_list, keypts_preds_refine)
        rep_coord_refine = self.offset_to_pts(center_list, reppts_preds_refine)
        init_boxes = [self.points2bbox(reppts_preds_init[i_lvl].detach()) * self.point_strides[i_lvl]
                      for i_lvl in range(len(reppts_preds_refine))]
        bbox_list = []
        for i_img, center in enumerate(center_list):
            bbox = []
            for i_lvl in range(len(reppts_preds_refine)):
                bbox_center = torch.cat([center[i_lvl][:, :2], center[i_lvl][:, :2]], dim=1)
                bbox.append(bbox_center + init_boxes[i_lvl][i_img].permute(1, 2, 0).reshape(-1, 4))
            bbox_list.append(bbox)
        if dense_ok(cfg.refine):
            targets_refine = point_target_kp_dense(bbox_list, gt_bboxes, gt_keypoints, cfg.refine, gt_labels_list=gt_labels,
                                                   valid_flag_list=None if all_valid else valid_flag_list)
        else:
            targets_refine = point_target_kp(bbox_list, valid_flag_list, gt_bboxes, gt_keypoints, img_metas, cfg.refine,
                                             gt_bboxes_ignore_list=gt_bboxes_ignore, gt_labels_list=gt_labels,
                                             label_channels=label_channels, sampling=self.sampling)
        (labels_list, label_weights_list, bbox_gt_list_refine, candidate_list_refine, bbox_weights_list_refine,
         keypoint_gt_list_refine, keypoint_weights_list_refine, num_total_pos_refine,
         num_total_neg_refine) = targets_refine
        num_total_samples_refine = (num_total_pos_refine + num_total_neg_refine
                                    if self.sampling else num_total_pos_refine)

        per_level = multi_apply(self.loss_single, cls_scores, kpt_coord_init, kpt_coord_refine, rep_coord_init,
                                rep_coord_refine, labels_list, label_weights_list, bbox_gt_list_init,
                                bbox_weights_list_init, bbox_gt_list_refine, bbox_weights_list_refine,
                                keypoint_gt_list_init, keypoint_weights_list_init, keypoint_gt_list_refine,
                                keypoint_weights_list_refine, self.point_strides,
                                num_total_samples_init=num_total_samples_init,
                                num_total_samples_refine=num_total_samples_refine)
        names = ['loss_cls', 'loss_bbox_init', 'loss_bbox_refine', 'loss_kpt_init', 'loss_kpt_refine']
        return dict(zip(names, per_level))

    # ------------------------------------------------------------------------------------------
    # detections from the refine stage: one whole-batch decode (decode.py), then NMS
    # ------------------------------------------------------------------------------------------
    def _decode(self, cls_scores, bbox_preds, kpt_preds, img_metas, cfg, rescale):
        # (true_divide: SER:730-733 divides by `new_tensor(scale_factor)`, where torch multiplies with the reciprocal for a
        #  python number -- one ulp off for factors like 1.5)
        return decode.decode_batch(self, cls_scores, bbox_preds, kpt_preds, img_metas, cfg, rescale, clamp_axis='landmark',
                                   true_divide=True)

    def get_bboxes(self, cls_scores, keypts_preds_init, keypts_preds_refine, reppts_preds_init, reppts_preds_refine,
                   img_metas, cfg, rescale=False, nms=True):
        """per image, per class NMS as in the reference (SER:667-750); the fused route is ``get_bboxes_packed_tensor``"""
        assert len(cls_scores) == len(keypts_preds_refine) == len(reppts_preds_refine)
        cls = [t.detach().float() for t in cls_scores]             # decode in fp32 under autocast
        box = [self.points2bbox(r.detach().float()) for r in reppts_preds_refine]
        kpt = [self.points2kpt(k.detach().float()) for k in keypts_preds_refine]
        return self.candidates_to_results(*self._decode(cls, box, kpt, img_metas, cfg, rescale), cfg, nms)

    def _packed_ok(self, cls_scores, img_metas, cfg, rescale):
        kind = cfg.nms.get('type', 'nms')
        if not (cls_scores[0].is_cuda and kind in ('nms', 'soft_nms') and self.use_sigmoid_cls and cfg.max_per_img > 0
                and rescale):      # (rescale=False leaves the landmarks [n, K, 3]: SER:730-734 reshapes only when rescaling)
            return False
        if not all(isinstance(m['scale_factor'], (int, float)) for m in img_metas):
            return False
        pre = cfg.get('nms_pre', -1)
        n = sum(min(c.shape[-2] * c.shape[-1], pre) if pre > 0 else c.shape[-2] * c.shape[-1] for c in cls_scores)
        C = self.cls_out_channels
        if kind == 'nms':
            return n <= 4096 and n * C <= 16384 and C <= 64
        if cfg.nms.get('method', 'linear') not in ('linear', 'gaussian'):
            return False
        from .postprocess import soft_nms_fused_supported
        return soft_nms_fused_supported(len(img_metas), n, C, cfg.max_per_img)

    def get_bboxes_packed(self, cls_scores, bbox_preds, kpt_preds, img_metas, cfg, rescale=True):
        """refine-stage maps, or pre-selected candidates (``decode.decode_level``) -> fixed-size device tensors (det [B,M,5],
        labels [B,M], landmarks [B,M,3K], count [B]): whole-batch decode + fused (soft-)NMS, no per-image / per-class Python
        loop and no host read before the results -- capturable as one HIP graph (detector.graphed_test_batch)"""
        from .postprocess import multiclass_nms_kp_fused, multiclass_soft_nms_kp_fused
        bboxes, scores, kpts = self._decode(cls_scores, bbox_preds, kpt_preds, img_metas, cfg, True)
        if cfg.nms.get('type', 'nms') == 'soft_nms':
            return multiclass_soft_nms_kp_fused(bboxes, scores, kpts, cfg.score_thr, cfg.nms, cfg.max_per_img)
        return multiclass_nms_kp_fused(bboxes, scores, kpts, cfg.score_thr, float(cfg.nms['iou_thr']), cfg.max_per_img)

    def get_bboxes_packed_tensor(self, cls_scores, keypts_preds_init, keypts_preds_refine, reppts_preds_init,
                                 reppts_preds_refine, img_metas, cfg, rescale=False):
        """The batch's detections as ONE device tensor [B, max_per_img, 7 + 3K] -- box (4), score, label, count (repeated),
        landmarks -- produced without any host read; None when the packed path does not apply."""
        cls = [t.float() for t in cls_scores]
        if not self._packed_ok(cls, img_metas, cfg, rescale):
            return None
        # The nms_pre candidates of a level are a function of its scores alone: choose them FIRST and convert only their rows
        # of the 588-channel point maps (get_bboxes, like the reference, converts every location of the map and then keeps
        # 1000: for a batch of 8 at 100 x 168 the float cast, the (y, x) -> (x, y) swap and the visibility column moved
        # ~1.5 GB).  Gathering rows commutes with the per-location arithmetic: same values.
        box, kpt, selected = [], [], []
        for i, c in enumerate(cls):
            B, n = c.shape[0], c.shape[2] * c.shape[3]
            scores = decode.class_scores(c)
            ctr = self.point_generators[i].grid_points(c.shape[-2:], self.point_strides[i], device=c.device)
            ctr = ctr[:, :2].unsqueeze(0).expand(B, -1, -1)
            rep, kp_ = reppts_preds_refine[i].detach().reshape(B, -1, n), keypts_preds_refine[i].detach().reshape(B, -1, n)
            top = decode.top_candidates(scores, cfg.get('nms_pre', -1))
            if top is not None:
                ctr, scores = decode.gather_rows(ctr, top), decode.gather_rows(scores, top)
                rep = torch.gather(rep, 2, top.unsqueeze(1).expand(B, rep.shape[1], -1))
                kp_ = torch.gather(kp_, 2, top.unsqueeze(1).expand(B, kp_.shape[1], -1))
            box.append(self.points2bbox(rep.float().unsqueeze(-1)))
            kpt.append(self.points2kpt(kp_.float().unsqueeze(-1)))
            selected.append((scores, ctr))
        return decode.pack_rows(*self.get_bboxes_packed(selected, box, kpt, img_metas, cfg, rescale))


@HEADS.register_module
class RepPointsHeadKpSerial(_RepPointsHeadKpTwoStage):
    """reppoints regressed from the keypoint maps (1x1 conv on keypts_out)"""
    parallel_reppts = False


@HEADS.register_module
class RepPointsHeadKpParallel(_RepPointsHeadKpTwoStage):
    """reppoints predicted by their own conv / deformable-conv branch"""
    parallel_reppts = True
