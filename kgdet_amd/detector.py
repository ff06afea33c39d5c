"""``RepPointsDetectorKp``: backbone -> neck -> keypoint-guided head, result packing.

Mirrors mmdet/models/detectors/reppoints_detector_kp.py:9-148 on top of
single_stage.py:9-70 and base.py:12-142 (``forward(img, img_meta, return_loss=True, **kw)``
dispatch, ``forward_train``, ``simple_test``, ``bbox2result_kp``).  The reference asserts one
image per GPU at test time (base.py:75-76); ``simple_test_batch`` lifts that for the batch-8
inference configuration, running decode + NMS for the whole batch at once.  ``aug_test`` is mmdetection's flip /
multi-scale test-time augmentation with the landmarks carried through (upstream reppoints_detector.py:27-82 semantics;
the reference's own ``aug_test`` at reppoints_detector_kp.py:118-148 cannot run).
"""
import numpy as np
import torch
import torch.nn as nn

from .registry import DETECTORS, build_backbone, build_head, build_neck


_PINNED_RESULTS = __import__('os').environ.get('KGDET_PINNED_RESULTS', '1') == '1'    # 0: `.cpu()` into pageable memory (A/B)


@DETECTORS.register_module
class RepPointsDetectorKp(nn.Module):

    def __init__(self, backbone, neck, bbox_head, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__()
        self.backbone = build_backbone(backbone)
        if neck is not None:
            self.neck = build_neck(neck)
        self.bbox_head = build_head(bbox_head)
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        self.init_weights(pretrained=pretrained)

    @property
    def with_neck(self):
        return hasattr(self, 'neck') and self.neck is not None

    @property
    def with_keypoint(self):
        return True

    def init_weights(self, pretrained=None):
        if isinstance(pretrained, str) and pretrained.startswith(('modelzoo://', 'open-mmlab://', 'http')):
            # there is no network: remote checkpoints cannot be fetched, weights stay randomly initialised
            pretrained = None
        self.backbone.init_weights(pretrained=pretrained)
        if self.with_neck:
            if isinstance(self.neck, nn.Sequential):
                for m in self.neck:
                    m.init_weights()
            else:
                self.neck.init_weights()
        self.bbox_head.init_weights()

    def extract_feat(self, img):
        x = self.backbone(img)
        if self.with_neck:
            x = self.neck(x)
        if not torch.is_grad_enabled() and not getattr(self.bbox_head, 'channels_last_inference', False):
            # the bf16 inference backbone runs channels-last (backbone.conv_bn); the head's kernels take NCHW
            # (a head whose towers stay channels-last -- heads_serial -- takes the maps as they come)
            x = tuple(o.contiguous() for o in x)
        return x

    def forward_dummy(self, img):
        return self.bbox_head(self.extract_feat(img), None)

    def train(self, mode=True):
        """``nn.Module.train`` + every derived inference-time copy of the weights dropped (autocast casts, folded backbone, packed
        deformable operands): they are keyed on the parameters' version counters, which a replayed HIP graph of the training
        step (``runner.GraphedTrainStep``) or a write through ``.data`` does not move.  ``eval()`` calls ``train(False)``."""
        from . import conv1x1
        conv1x1.invalidate_inference_caches()
        return super(RepPointsDetectorKp, self).train(mode)

    def forward_train(self, img, img_metas, gt_bboxes, gt_labels, gt_keypoints, gt_bboxes_ignore=None, gt_table=None):
        """``gt_table``: the device table of a ``static_batch.StaticBatch`` (ground-truth counts and valid extents in device
        memory, ground truth in buffers of fixed capacity); the KGDet head only -- any other head raises
        ``NotImplementedError``"""
        from . import conv1x1
        if gt_table is not None and not getattr(self.bbox_head, 'takes_gt_table', False):
            raise NotImplementedError('%s takes no ground-truth table (the KGDet head does)' % type(self.bbox_head).__name__)
        with conv1x1.step_scope():    # the split-bf16 convolutions' weight images: one pack launch per step
            x = self.extract_feat(img)
            outs = self.bbox_head(x, img_metas)
        loss_inputs = outs + (gt_bboxes, gt_labels, gt_keypoints, img_metas, self.train_cfg)
        if gt_table is None:
            return self.bbox_head.loss(*loss_inputs, gt_bboxes_ignore=gt_bboxes_ignore)
        return self.bbox_head.loss(*loss_inputs, gt_bboxes_ignore=gt_bboxes_ignore, gt_table=gt_table)

    def bbox2result_kp(self, bboxes, labels, kpts, num_classes):
        """per-class numpy lists: (bboxes_in_cls, bbox_scores, kpt_in_cls), or a 1-tuple when empty"""
        if bboxes.shape[0] == 0:
            return ([np.zeros((0, 5), dtype=np.float32) for i in range(num_classes - 1)], )
        # (no use of ``self``: runner.DeviceResults.to_host calls this without a detector)
        if torch.is_tensor(bboxes):
            bboxes, labels, kpts = bboxes.float().cpu().numpy(), labels.cpu().numpy(), kpts.float().cpu().numpy()
        return ([bboxes[labels == i, :] for i in range(num_classes - 1)], bboxes[:, 4],
                [kpts[labels == i, :] for i in range(num_classes - 1)])

    def simple_test_batch(self, img, img_meta, rescale=False):
        x = self.extract_feat(img)
        outs = self.bbox_head(x, img_meta)
        get = getattr(self.bbox_head, 'get_bboxes_numpy', self.bbox_head.get_bboxes)   # one D2H copy per batch
        bbox_list = get(*(outs + (img_meta, self.test_cfg, rescale)))
        return [self.bbox2result_kp(det_bboxes, det_labels, det_kpts, self.bbox_head.num_classes)
                for det_bboxes, det_labels, det_kpts in bbox_list]

    def pack_detections(self, det, labels, kpts, max_per_img):
        """(det [n, 5], labels [n], kpts [n, 3K]) device tensors -> one block [1, max_per_img, 7 + 3K] float32 in the column
        layout of ``get_bboxes_packed_tensor`` (box, score, label, count, landmarks), with torch ops on their device; rows from
        ``n`` on are left unwritten.  More than ``max_per_img`` detections: ``NotImplementedError`` (never cut silently)."""
        n = int(det.shape[0])
        if n > max_per_img:
            raise NotImplementedError('%d detections for an image, but the device results hold max_per_img = %d rows'
                                      % (n, max_per_img))
        kpts = kpts.flatten(1) if kpts.dim() > 2 else kpts
        block = torch.empty((1, max_per_img, 7 + kpts.shape[1]), dtype=torch.float32, device=det.device)
        block[0, :, 6] = n
        block[0, :n, :5] = det.float()
        block[0, :n, 5] = labels.float()
        block[0, :n, 7:] = kpts.float()
        return block

    def simple_test_batch_device(self, img, img_meta, rescale=False):
        """``simple_test_batch`` without the download: the batch's detections as the device tensor [B, max_per_img, 7 + 3K] of
        ``get_bboxes_packed_tensor``; where the head's packed post-processing does not apply, ``get_bboxes``'s per-image
        tensors written into the same layout (``pack_detections``)"""
        M = int(self.test_cfg.max_per_img)
        if M <= 0:
            raise NotImplementedError('device results need test_cfg.max_per_img > 0 (the rows per image)')
        x = self.extract_feat(img)
        outs = self.bbox_head(x, img_meta)
        packed = self.bbox_head.get_bboxes_packed_tensor(*(outs + (img_meta, self.test_cfg, rescale)))
        if packed is None:
            bbox_list = self.bbox_head.get_bboxes(*(outs + (img_meta, self.test_cfg, rescale)))
            packed = torch.cat([self.pack_detections(d, lab, k, M) for d, lab, k in bbox_list])
        return packed

    def aug_test_device(self, imgs, img_metas, rescale=False):
        """``aug_test`` with the merged detections left on the device: one block [1, max_per_img, 7 + 3K]"""
        if int(self.test_cfg.max_per_img) <= 0:
            raise NotImplementedError('device results need test_cfg.max_per_img > 0 (the rows per image)')
        det, labels, kp = self.merge_aug_detections(self.aug_candidates(imgs, img_metas), img_metas, rescale)
        return self.pack_detections(det, labels, kp, int(self.test_cfg.max_per_img))

    def graphed_test_batch(self, img, img_meta, rescale=False, autocast_dtype=None, warmup=3):
        """``simple_test_batch`` for a fixed input shape and fixed image metas as ONE HIP-graph launch.

        A batch is ~360 kernel launches whose CPU-side issue (Python module calls + launch latency) takes about as
        long as the GPU needs to run them; backbone, neck, head, decode and the fused NMS have no host read, so the
        whole chain is captured once (``torch.cuda.CUDAGraph`` = hipGraph) and replayed per batch, followed by the
        single device->host copy of the packed results.  Returns ``run(img) -> results`` (same results as
        ``simple_test_batch``); ``run.static_img`` is the graph's input buffer -- ``run(run.static_img)`` after writing the
        batch into it (e.g. as the destination of the loader's host->device copy) skips the 103 MB device copy; raises NotImplementedError when the head's packed post-processing does not apply."""
        import contextlib
        assert img.is_cuda and not self.training
        scope = (lambda: torch.autocast('cuda', dtype=autocast_dtype)) if autocast_dtype is not None \
            else contextlib.nullcontext
        static_img = img.clone()

        def chain():
            outs = self.bbox_head(self.extract_feat(static_img), img_meta)
            return self.bbox_head.get_bboxes_packed_tensor(*(outs + (img_meta, self.test_cfg, rescale)))

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad(), scope():
            for _ in range(warmup):          # MIOpen find, lazy module loads, weight caches: all before the capture
                packed = chain()
        torch.cuda.current_stream().wait_stream(side)
        if packed is None:
            raise NotImplementedError('packed post-processing not applicable to this head / test_cfg / metas')
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), scope(), torch.cuda.graph(graph):
            static_out = chain()
        num_classes = self.bbox_head.num_classes

        # the results land in a page-locked buffer (a `.cpu()` into pageable memory is staged by the driver: 232 us for the
        # 2.8 MB of a batch of 8 against ~60); bbox2result_kp copies the valid rows out of it, so it is reused per batch
        host_out = torch.empty(static_out.shape, dtype=static_out.dtype, pin_memory=True)

        def run(new_img):
            if new_img is not static_img:       # (run.static_img IS the input buffer: a loader that writes into it saves the copy)
                static_img.copy_(new_img)
            graph.replay()
            if _PINNED_RESULTS:
                host_out.copy_(static_out, non_blocking=True)
                torch.cuda.current_stream().synchronize()
                dets = self.bbox_head.unpack_results(host_out.numpy())
            else:
                dets = self.bbox_head.unpack_results(static_out.cpu().numpy())
            # (d.copy(): the score column of the result is a view of d; labels and the per-class rows are copies already)
            return [self.bbox2result_kp(d.copy(), lab, k, num_classes) for d, lab, k in dets]

        # Pipelined use (a serving loop): ``slot = run.submit()`` replays the graph on the batch in ``run.static_img`` and starts
        # the device->host copy of its packed results on a side stream; ``run.collect(slot)`` waits for that copy and unpacks.
        # Calling submit(k + 1) before collect(k) puts batch k's copy and host-side unpacking UNDER batch k + 1's kernels (the
        # serial ``run`` leaves the GPU idle for both).  Two result slots: collect(k) must have returned before submit(k + 2).
        stash = [torch.empty_like(static_out) for _ in range(2)]
        hosts = [torch.empty(static_out.shape, dtype=static_out.dtype, pin_memory=True) for _ in range(2)]
        ready = [torch.cuda.Event() for _ in range(2)]
        landed = [torch.cuda.Event() for _ in range(2)]
        copy_stream = torch.cuda.Stream()
        counter = [0]

        def submit(new_img=None):
            if new_img is not None and new_img is not static_img:
                static_img.copy_(new_img)
            slot = counter[0] & 1
            counter[0] += 1
            graph.replay()
            stash[slot].copy_(static_out)              # (2.8 MB device copy: the next replay overwrites static_out)
            ready[slot].record()
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(ready[slot])
                hosts[slot].copy_(stash[slot], non_blocking=True)
                landed[slot].record()
            return slot

        def collect(slot):
            landed[slot].synchronize()
            dets = self.bbox_head.unpack_results(hosts[slot].numpy())
            return [self.bbox2result_kp(d.copy(), lab, k, num_classes) for d, lab, k in dets]

        run.submit, run.collect = submit, collect
        run.graph, run.static_img, run.static_out = graph, static_img, static_out
        # The captured kernels hold raw pointers into the module-level weight-image caches (packed deformable-conv
        # operands, folded conv+BN weights).  Those caches are cleared on mode switches / when they fill up, which
        # would free memory the graph still reads: the graph keeps its own strong references.
        from . import backbone, dcn
        run.pinned = ([v[2] for v in dcn._pack_cache.values()], [(v.weight, v.bias, v.packed) for v in backbone._fold_cache.values()])
        return run

    def simple_test(self, img, img_meta, rescale=False):
        return self.simple_test_batch(img, img_meta, rescale)[0]

    def aug_candidates(self, imgs, img_metas):
        """every augmentation's decoded candidates in its own resized frame: a list, in the order of ``imgs``, of
        (bboxes [n,4], scores [n,1+C], kpts [n,K,3]) from ``get_bboxes(..., rescale=False, nms=False)``.  Augmentations
        with the same tensor shape (an image and its flip always) share one forward pass."""
        metas = [m[0] for m in img_metas]
        groups = {}
        for i, t in enumerate(imgs):
            groups.setdefault(tuple(t.shape[1:]), []).append(i)
        cands = [None] * len(imgs)
        for idx in groups.values():
            img = imgs[idx[0]] if len(idx) == 1 else torch.cat([imgs[i] for i in idx])
            group_metas = [metas[i] for i in idx]
            outs = self.bbox_head(self.extract_feat(img), group_metas)
            for i, c in zip(idx, self.bbox_head.get_bboxes(*(outs + (group_metas, self.test_cfg, False, False)))):
                cands[i] = c
        return cands

    def merge_aug_detections(self, cands, img_metas, rescale=False):
        """steps after ``aug_candidates``: map back + merge (``kgdet_aug_merge`` for GPU candidates, the restatement
        ``merge_aug_results_kp`` for host ones), NMS on the merged set, the rescale of ``aug_test``;
        returns (det [k,5], labels [k], kpts [k,3K])"""
        from .postprocess import aug_merge_kp, aug_nms_kp, aug_scale_factor
        metas = [m[0] for m in img_metas]
        for m in metas:
            aug_scale_factor(m)                     # NotImplementedError for a per-axis scale factor
        merge = aug_merge_kp if cands[0][0].is_cuda else merge_aug_results_kp
        bboxes, scores, kpts = merge([c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands], metas)
        det, labels, kp = aug_nms_kp(bboxes, scores, kpts.reshape(kpts.shape[0], -1), self.test_cfg)
        return rescale_aug_detections(det, labels, kp, metas[0], rescale)

    def aug_test(self, imgs, img_metas, rescale=False):
        """test-time augmentation: ``imgs`` A tensors [1,3,H_a,W_a], ``img_metas`` A lists of one meta (``flip``,
        ``scale_factor``, ``img_shape``, ``flip_indices``).  Each augmentation is decoded in its own frame, mapped back to
        the original image, all of them are merged and go through the test_cfg's NMS together; the result has the format
        of ``simple_test``."""
        det, labels, kp = self.merge_aug_detections(self.aug_candidates(imgs, img_metas), img_metas, rescale)
        return self.bbox2result_kp(det, labels, kp, self.bbox_head.num_classes)

    def forward_test(self, imgs, img_metas, **kwargs):
        # (runner._RowSink.single repeats these checks and this dispatch for device results: keep the two in step)
        for var, name in [(imgs, 'imgs'), (img_metas, 'img_metas')]:
            if not isinstance(var, list):
                raise TypeError('{} must be a list, but got {}'.format(name, type(var)))
        num_augs = len(imgs)
        if num_augs != len(img_metas):
            raise ValueError('num of augmentations ({}) != num of image meta ({})'.format(len(imgs), len(img_metas)))
        imgs_per_gpu = imgs[0].size(0)
        assert imgs_per_gpu == 1
        if num_augs == 1:
            return self.simple_test(imgs[0], img_metas[0], **kwargs)
        return self.aug_test(imgs, img_metas, **kwargs)

    def forward(self, img, img_meta, return_loss=True, **kwargs):
        if return_loss:
            return self.forward_train(img, img_meta, **kwargs)
        return self.forward_test(img, img_meta, **kwargs)

    def show_result(self, data, result, img_norm_cfg, dataset=None, score_thr=0.3):
        """base.py:90-142 without the window: ``data['img'][0]`` (one test sample's normalised tensor, [3, H, W] or collated
        [B, 3, H, W], with its metas in ``data['img_meta'][0]``) is denormalised, cut to ``img_shape`` and drawn with ``result``
        as it stands (not rescaled: a result of ``rescale=False`` lies in this frame), landmarks included -> the list of uint8
        RGB arrays.  ``dataset``: None for ``self.CLASSES``, or a sequence of class names; a dataset-name string (the
        reference's ``get_classes``) raises ``TypeError``."""
        from .visualize import denormalize, show_result
        if dataset is None:
            class_names = self.CLASSES
        elif isinstance(dataset, (list, tuple)):
            class_names = dataset
        else:
            raise TypeError('dataset must be a valid type, but got {} (a sequence of class names, or None)'.format(type(dataset)))
        imgs, metas = data['img'][0], data['img_meta'][0]
        if imgs.dim() == 3:
            imgs, metas = imgs[None], [metas]
        elif isinstance(metas, dict):
            metas = [metas]
        results = result if isinstance(result, list) else [result] * len(metas)
        out = []
        for img, meta, res in zip(imgs.float().cpu().numpy(), metas, results):
            h, w = meta['img_shape'][:2]
            shown = denormalize(img, **img_norm_cfg)[:h, :w]
            out.append(show_result(np.ascontiguousarray(shown), res, class_names, score_thr=score_thr))
        return out


def merge_aug_results_kp(aug_bboxes, aug_scores, aug_kpts, img_metas):
    """The pure-torch statement of the test-time merge (upstream ``merge_aug_results`` + ``bbox_mapping_back``,
    mmdet/core/bbox/transforms.py:71-103, with the landmarks carried through); any device.

    Per augmentation (meta: ``img_shape``, scalar ``scale_factor`` s, ``flip``, ``flip_indices``): a flip maps
    x1' = (w - x2) - 1, x2' = (w - x1) - 1 and every landmark x' = (w - x) - 1 with w = img_shape[1], and GATHERS the
    landmarks: out slot k takes the landmark of input slot perm[k], perm = flip_indices[0::2] // 2 (``flip_perm`` only lets
    involutions through, for which that is also "slot k moves to slot perm[k]"); then box coordinates and landmark x, y are
    divided by s.  Visibility and scores are unchanged.  The rows are concatenated in augmentation order.

    The division is torch's: on a GPU ``x / s`` is ``x * float32(1 / s)`` (the reciprocal taken in double, rounded once), on
    the CPU a true division.  The two agree bit for bit where 1 / s is a float32 (s = 0.5, 1, 2, ...) and otherwise in all but
    the last bit: both lie within ``2 U |x / s|`` (+ the two roundings of a flip), U = 2^-24, of the exact quotient
    (tests/aug_merge_cases.py counts the bound; at s = 1.666 a third of the coordinates differ in that bit).  The kernel
    (``postprocess.aug_merge_kp``) is bit-identical to this function on GPU tensors, and within that bound of it on CPU tensors.
    aug_bboxes [n,4], aug_scores [n,1+C], aug_kpts [n,K,3] per augmentation -> (bboxes [T,4], scores [T,1+C], kpts [T,K,3])."""
    from .postprocess import aug_scale_factor, flip_perm
    out_b, out_k = [], []
    for bboxes, kpts, meta in zip(aug_bboxes, aug_kpts, img_metas):
        sf = aug_scale_factor(meta)
        if kpts.dim() == 2:
            kpts = kpts.reshape(kpts.shape[0], kpts.shape[1] // 3, 3)
        if meta['flip']:
            w = float(meta['img_shape'][1])
            bboxes = torch.stack([(w - bboxes[:, 2]) - 1, bboxes[:, 1], (w - bboxes[:, 0]) - 1, bboxes[:, 3]], dim=1)
            kpts = kpts[:, flip_perm(meta['flip_indices'], kpts.device)]
            kpts = torch.stack([(w - kpts[..., 0]) - 1, kpts[..., 1], kpts[..., 2]], dim=-1)
        out_b.append(bboxes / sf)
        out_k.append(torch.cat([kpts[..., :2] / sf, kpts[..., 2:]], dim=-1))
    return torch.cat(out_b), torch.cat(list(aug_scores)), torch.cat(out_k)


def rescale_aug_detections(det, labels, kpts, meta, rescale):
    """the last step of ``aug_test``: merged detections stay in the original frame when ``rescale``, otherwise box
    coordinates and landmark x, y are multiplied by the first augmentation's scale factor (reppoints_detector.py:74-78)"""
    if rescale:
        return det, labels, kpts
    from .postprocess import aug_scale_factor
    sf = aug_scale_factor(meta)
    k = kpts.reshape(kpts.shape[0], -1, 3)
    k = torch.cat([k[..., :2] * sf, k[..., 2:]], dim=-1).reshape(kpts.shape)
    return torch.cat([det[:, :4] * sf, det[:, 4:]], dim=1), labels, k
