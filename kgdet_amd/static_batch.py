"""Fixed input buffers for the training step on REAL batches: one set of tensors, at fixed addresses and of fixed shapes, that
holds whichever batch comes next.

A captured step bakes the addresses and shapes of its inputs into its launches (``runner.GraphedTrainStep`` replays batches
of ONE shape, with the same number of ground-truth rows per image).  Real batches differ in two ways: every image has its own
number of garments, and a batch collated to ``(1333, 800)`` with ``size_divisor=32`` has its own padded size per orientation.
A ``StaticBatch`` holds

    ``img``              [B, 3, H, W] float32   the canvas
    ``gt_bboxes[b]``     [cap, 4]     float32
    ``gt_labels[b]``     [cap]        int64
    ``gt_keypoints[b]``  [cap, K, 3]  float32
    ``table``            [B, 4]       int32     (num_gt, valid_h, valid_w, 0) per image, read by the head-loss kernels

and ``load(batch)`` copies any batch that fits into them: the image into the canvas's top-left corner (the rest zeroed), the
first ``num_gt`` rows of each ground-truth tensor (later rows may hold anything: the kernels never read them), and the table.

Semantics: a batch on a canvas is that batch collated to a larger common size.  mmdetection does the same to the smaller images
of any batch (``datasets.collate`` pads to the largest): the convolutions see zero pixels below and right of each image, each
image's own ``pad_shape`` still decides which grid points are valid for the assigner and the losses.  The step's results equal
the eager step on the same canvas tensor; they do not equal the eager step on the tight batch tensor (the zero border moves
the backbone's outputs near the image's edge).

With these buffers nothing in ``forward_train(..., gt_table=)`` depends on the batch but the CONTENTS of device memory
(``tests/test_gpu_head_loss_table.py`` replays a captured forward + backward of the head loss on other counts, extents and
maps).  Driving ``GraphedTrainStep`` and ``Runner`` from them is not part of this module yet.

``check`` and ``table_of`` are host functions and need no GPU (a ``StaticBatch`` built with ``device=None`` has no buffers).
"""
import numpy as np
import torch

from .head_loss import MAX_GT, MAX_IMAGES, MAX_POINTS

TABLE_RING = 8     # page-locked copies of the table: the host may run this many loads ahead of the device


def metas_of(batch):
    """the per-image metas of a batch dict, under either of the two keys in use (``img_meta``: ``datasets.collate`` and
    ``forward``; ``img_metas``: ``forward_train``)"""
    return batch['img_meta'] if 'img_meta' in batch else batch['img_metas']


class StaticBatch(object):
    def __init__(self, num_images, canvas, gt_capacity, num_keypoints, stride, pos_num, device=None):
        """``canvas``: (H, W) of the image buffer, multiples of ``stride`` (the one pyramid level's); ``gt_capacity``: rows of
        every ground-truth buffer (1..64); ``pos_num``: the PointAssigner's; ``device=None``: no buffers (``check`` /
        ``table_of`` only)"""
        H, W = int(canvas[0]), int(canvas[1])
        self.B, self.canvas, self.cap = int(num_images), (H, W), int(gt_capacity)
        self.K, self.stride, self.pos_num = int(num_keypoints), int(stride), int(pos_num)
        if not 1 <= self.B <= MAX_IMAGES:
            raise ValueError('1..%d images per batch, not %d' % (MAX_IMAGES, self.B))
        if not 1 <= self.cap <= MAX_GT:
            raise ValueError('a ground-truth capacity of 1..%d rows, not %d' % (MAX_GT, self.cap))
        if H <= 0 or W <= 0 or H % self.stride or W % self.stride:
            raise ValueError('the canvas %s must be positive multiples of the stride %d' % ((H, W), self.stride))
        self.grid = (H // self.stride, W // self.stride)
        if self.grid[0] * self.grid[1] > MAX_POINTS or self.grid[0] * self.grid[1] < self.pos_num:
            raise ValueError('a grid of %d x %d points: at least pos_num = %d and at most %d' %
                             (self.grid + (self.pos_num, MAX_POINTS)))
        self.device = None if device is None else torch.device(device)
        self.img = self.table = None
        self.gt_bboxes, self.gt_labels, self.gt_keypoints = [], [], []
        self.img_meta = [None] * self.B       # the metas of the batch in the buffers (host data, replaced by every load)
        self.loads = 0
        if self.device is not None:
            dev = self.device
            self.img = torch.zeros((self.B, 3, H, W), dtype=torch.float32, device=dev)
            for _ in range(self.B):
                self.gt_bboxes.append(torch.zeros((self.cap, 4), dtype=torch.float32, device=dev))
                self.gt_labels.append(torch.zeros((self.cap, ), dtype=torch.int64, device=dev))
                self.gt_keypoints.append(torch.zeros((self.cap, self.K, 3), dtype=torch.float32, device=dev))
            self.table = torch.zeros((self.B, 4), dtype=torch.int32, device=dev)
            # the table reaches the device from page-locked memory; slot k % TABLE_RING belongs to load k, and the event of the
            # copy that last read a slot is waited for before the slot is rewritten (only when the host ran a ring ahead)
            self._ring = torch.zeros((TABLE_RING, self.B, 4), dtype=torch.int32).pin_memory()
            self._ring_events = [None] * TABLE_RING
            self._filled = (0, 0)             # the part of the canvas the last load wrote pixels to

    @classmethod
    def for_model(cls, model, num_images, canvas, gt_capacity, device=None):
        """the static batch of a detector with the KGDet head (one level): stride, keypoints and pos_num are the model's"""
        target = model.module if hasattr(model, 'module') else model
        head = target.bbox_head
        if not getattr(head, 'takes_gt_table', False) or len(head.point_strides) != 1:
            raise NotImplementedError('a static batch feeds the KGDet head (one level); %s reads its ground-truth counts on the '
                                      'host' % type(head).__name__)
        pos_num = int(target.train_cfg.uniform.assigner.get('pos_num', 3))
        return cls(num_images, canvas, gt_capacity, head.num_keypts, head.point_strides[0], pos_num, device)

    # ---------------------------------------------------------------------------------------------- host side
    def extent_of(self, meta):
        """(rows, columns) of the grid inside the image's own pad_shape: ``heads.py``'s expression"""
        s = self.stride
        return (min(int(np.ceil(meta['pad_shape'][0] / s)), self.grid[0]),
                min(int(np.ceil(meta['pad_shape'][1] / s)), self.grid[1]))

    def check(self, batch):
        """``ValueError`` unless ``load(batch)`` can hold the batch; reads shapes, dtypes and metas only, copies nothing"""
        img = batch['img']
        if img.dim() != 4 or img.shape[0] != self.B or img.shape[1] != 3:
            raise ValueError('a batch of %d images [%d, 3, h, w] is expected, got %s' % (self.B, self.B, tuple(img.shape)))
        if img.dtype != torch.float32:
            raise ValueError('the image tensor must be float32, not %s' % img.dtype)
        if img.shape[2] > self.canvas[0] or img.shape[3] > self.canvas[1]:
            raise ValueError('the batch image %s is larger than the canvas %s' % (tuple(img.shape[2:]), self.canvas))
        ignore = batch.get('gt_bboxes_ignore')
        if ignore is not None and any(g is not None for g in ignore):
            raise ValueError('the batch carries gt_bboxes_ignore: the static batch has no buffer for ignore regions (the '
                             'configs train with_crowd=False)')
        metas = metas_of(batch)
        lists = [batch['gt_bboxes'], batch['gt_labels'], batch['gt_keypoints'], metas]
        if any(len(l) != self.B for l in lists):
            raise ValueError('every per-image list must hold %d entries' % self.B)
        for b in range(self.B):
            bb, lab, kp = batch['gt_bboxes'][b], batch['gt_labels'][b], batch['gt_keypoints'][b]
            n = int(bb.shape[0])
            if n == 0:
                raise ValueError('No gt or bboxes')
            if n > self.cap:
                raise ValueError('image %d has %d ground truths, the capacity is %d' % (b, n, self.cap))
            if bb.dtype != torch.float32 or kp.dtype != torch.float32 or lab.dtype != torch.int64:
                raise ValueError('image %d: boxes and keypoints must be float32 and labels int64, not %s / %s / %s' %
                                 (b, bb.dtype, kp.dtype, lab.dtype))
            if tuple(bb.shape) != (n, 4) or tuple(lab.shape) != (n, ) or tuple(kp.shape) != (n, self.K, 3):
                raise ValueError('image %d: ground truth of shapes %s / %s / %s, expected [n, 4] / [n] / [n, %d, 3]' %
                                 (b, tuple(bb.shape), tuple(lab.shape), tuple(kp.shape), self.K))
            vh, vw = self.extent_of(metas[b])
            if vh * vw < self.pos_num:
                raise ValueError('image %d: its pad_shape %s holds %d grid points, fewer than pos_num = %d' %
                                 (b, tuple(metas[b]['pad_shape'][:2]), vh * vw, self.pos_num))

    def table_of(self, batch):
        """the host table int32 [B, 4] = (num_gt, valid_h, valid_w, 0): the extents are min(ceil(pad_shape / stride), grid)"""
        metas = metas_of(batch)
        table = np.zeros((self.B, 4), dtype=np.int32)
        for b in range(self.B):
            table[b, 0] = int(batch['gt_bboxes'][b].shape[0])
            table[b, 1], table[b, 2] = self.extent_of(metas[b])
        return table

    # ---------------------------------------------------------------------------------------------- device side
    def load(self, batch):
        """copy a batch (``datasets.collate`` / ``collate_device`` + the usual move to the device; host or device tensors)
        into the buffers.  ``batch['img'] is self.img`` -- a caller that had ``DeviceImageTransform`` write the canvas through
        ``out=`` -- skips the image copy: such a caller leaves zeros beyond every image's pad_shape itself."""
        self.check(batch)
        dev = self.device
        img = batch['img']
        H, W = self.canvas
        with torch.no_grad():
            if img is not self.img:
                h, w = int(img.shape[2]), int(img.shape[3])
                # the rest of the canvas is zeroed where the previous load left pixels: a smaller batch after a larger one
                # must not see stale ones
                fh, fw = self._filled
                if fh > h:
                    self.img[:, :, h:fh, :].zero_()
                if fw > w:
                    self.img[:, :, :h, w:fw].zero_()
                self.img[:, :, :h, :w].copy_(img, non_blocking=True)
                self._filled = (h, w)
            else:
                self._filled = (H, W)
            dst, src = [], []
            for b in range(self.B):
                n = int(batch['gt_bboxes'][b].shape[0])
                for buf, key in ((self.gt_bboxes, 'gt_bboxes'), (self.gt_labels, 'gt_labels'), (self.gt_keypoints, 'gt_keypoints')):
                    dst.append(buf[b][:n])
                    src.append(batch[key][b].to(dev, non_blocking=True))
            torch._foreach_copy_(dst, src)
            slot = self.loads % TABLE_RING
            ev = self._ring_events[slot]
            if ev is not None:
                ev.synchronize()
            self._ring[slot].copy_(torch.from_numpy(self.table_of(batch)))
            self.table.copy_(self._ring[slot], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._ring_events[slot] = ev
        self.loads += 1
        self.img_meta[:] = list(metas_of(batch))
        return self

    def as_batch(self):
        """the dict ``forward`` / ``batch_processor`` take: the buffers themselves (the same objects after every load)"""
        return dict(img=self.img, img_meta=self.img_meta, gt_bboxes=self.gt_bboxes, gt_labels=self.gt_labels,
                    gt_keypoints=self.gt_keypoints, gt_table=self.table)
