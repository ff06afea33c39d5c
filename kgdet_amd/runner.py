"""Training runtime of the KGDet configs without mmcv  (SURVEY 8f row 3).

What the reference gets from ``mmcv==0.2.13``'s ``Runner`` + hooks (third-party, not in the reference tree; pinned by
``requirements.txt:7``) and ``mmdet/apis/train.py``, restated as one small loop:

* ``parse_losses`` / ``batch_processor`` / ``build_optimizer``  -- ``mmdet/apis/train.py:17-134``.
* ``LrSchedule`` -- mmcv's ``LrUpdaterHook`` for ``lr_config = dict(policy='step', warmup='linear', warmup_iters=500,
  warmup_ratio=1/3, step=[8, 11])`` (``configs/kgdet_moment_r50_fpn_1x-demo.py:134-139``): the regular rate is
  ``base_lr * gamma ** (#steps already passed)`` set at the start of every epoch; during the first ``warmup_iters``
  iterations it is scaled by ``1 - (1 - it / warmup_iters) * (1 - warmup_ratio)`` ('linear'), ``warmup_ratio``
  ('constant') or ``warmup_ratio ** (1 - it / warmup_iters)`` ('exp'); at ``it == warmup_iters`` it returns to the
  regular rate.
* ``Runner`` -- epoch loop, ``DistOptimizerHook`` (all-reduce + grad-clip 35 + step), checkpoint every ``interval``
  epochs as ``epoch_{n}.pth`` + ``latest.pth`` with ``meta = {epoch, iter}`` and the optimizer state, ``resume``.
* ``single_gpu_test`` / ``multi_gpu_test`` / ``collect_results`` -- ``mmdetection/tools/test.py:18-100``: inference over a
  dataset, sharded by rank (sample i of the padded index list goes to rank i % world_size, the ``DistributedSampler(shuffle=False)``
  of ``mmdet/datasets/loader/build_loader.py``), results gathered on rank 0 in dataset order, padding samples dropped.
"""
import os
import shutil
import time
from collections import OrderedDict

import torch

from .checkpoint import load_checkpoint, save_checkpoint
from .dist import DistOptimizerHook


def parse_losses(losses):
    log_vars = OrderedDict()
    for name, value in losses.items():
        if isinstance(value, torch.Tensor):
            log_vars[name] = value.mean()
        elif isinstance(value, list):
            log_vars[name] = sum(v.mean() for v in value)
        else:
            raise TypeError('{} is not a tensor or list of tensors'.format(name))
    loss = sum(v for k, v in log_vars.items() if 'loss' in k)
    log_vars['loss'] = loss
    return loss, log_vars


def batch_processor(model, data, train_mode=True):
    losses = model(**data)
    loss, log_vars = parse_losses(losses)
    return dict(loss=loss, log_vars=log_vars, num_samples=len(data['img']))


def build_optimizer(model, optimizer_cfg):
    import re
    model = model.module if hasattr(model, 'module') else model
    cfg = dict(optimizer_cfg)
    paramwise = cfg.pop('paramwise_options', None)
    cls = getattr(torch.optim, cfg.pop('type'))
    if paramwise is None:
        return cls(model.parameters(), **cfg)
    base_lr, base_wd = cfg['lr'], cfg.get('weight_decay', None)
    if 'bias_decay_mult' in paramwise or 'norm_decay_mult' in paramwise:
        assert base_wd is not None
    groups = []
    for name, param in model.named_parameters():
        group = {'params': [param]}
        if param.requires_grad:
            if re.search(r'(bn|gn)(\d+)?.(weight|bias)', name):
                if base_wd is not None:
                    group['weight_decay'] = base_wd * paramwise.get('norm_decay_mult', 1.)
            elif name.endswith('.bias'):
                group['lr'] = base_lr * paramwise.get('bias_lr_mult', 1.)
                if base_wd is not None:
                    group['weight_decay'] = base_wd * paramwise.get('bias_decay_mult', 1.)
        groups.append(group)
    return cls(groups, **cfg)


class LrSchedule(object):
    def __init__(self, policy='step', step=(), gamma=0.1, by_epoch=True, warmup=None, warmup_iters=0,
                 warmup_ratio=0.1, **unused):
        if policy != 'step':
            raise NotImplementedError('lr policy {!r} (the KGDet configs use "step")'.format(policy))
        if warmup is not None:
            if warmup not in ('constant', 'linear', 'exp'):
                raise ValueError('"{}" is not a supported type for warming up'.format(warmup))
            assert warmup_iters > 0 and 0 < warmup_ratio <= 1.0
        self.step = step if isinstance(step, int) else list(step)
        assert (self.step > 0) if isinstance(self.step, int) else all(s > 0 for s in self.step)
        self.gamma, self.by_epoch = gamma, by_epoch
        self.warmup, self.warmup_iters, self.warmup_ratio = warmup, warmup_iters, warmup_ratio
        self.base_lr, self.regular_lr = [], []

    def before_run(self, optimizer):
        for g in optimizer.param_groups:
            g.setdefault('initial_lr', g['lr'])
        self.base_lr = [g['initial_lr'] for g in optimizer.param_groups]

    def regular(self, progress):
        if isinstance(self.step, int):
            return [lr * self.gamma ** (progress // self.step) for lr in self.base_lr]
        passed = len(self.step)
        for i, s in enumerate(self.step):
            if progress < s:
                passed = i
                break
        return [lr * self.gamma ** passed for lr in self.base_lr]

    def warm(self, cur_iter):
        if self.warmup == 'constant':
            k = self.warmup_ratio
        elif self.warmup == 'linear':
            k = 1 - (1 - cur_iter / self.warmup_iters) * (1 - self.warmup_ratio)
        else:
            k = self.warmup_ratio ** (1 - cur_iter / self.warmup_iters)
        return [lr * k for lr in self.regular_lr]

    @staticmethod
    def _set(optimizer, lrs):
        for g, lr in zip(optimizer.param_groups, lrs):
            g['lr'] = lr

    def before_train_epoch(self, optimizer, epoch):
        if self.by_epoch:
            self.regular_lr = self.regular(epoch)
            self._set(optimizer, self.regular_lr)

    def before_train_iter(self, optimizer, cur_iter):
        if not self.by_epoch:
            self.regular_lr = self.regular(cur_iter)
            if self.warmup is None or cur_iter >= self.warmup_iters:
                self._set(optimizer, self.regular_lr)
            else:
                self._set(optimizer, self.warm(cur_iter))
        elif self.warmup is not None and cur_iter <= self.warmup_iters:
            self._set(optimizer, self.regular_lr if cur_iter == self.warmup_iters else self.warm(cur_iter))


def test_shard(n, world_size, rank):
    """Indices of rank ``rank``: the reference's test-time ``DistributedSampler(dataset, world_size, rank, shuffle=False)`` -- the
    index list padded by wrapping to a multiple of ``world_size``, then every ``world_size``-th index from ``rank`` on."""
    total = int(-(-n // world_size)) * world_size
    idx = list(range(n))
    if n > 0:
        idx = (idx * (-(-total // n)))[:total]      # (wrapping as often as needed: n < world_size / 2 leaves no rank empty)
    assert len(idx) == total or n == 0
    return idx[rank:total:world_size]


class DeviceResults(object):
    """What ``single_gpu_test(..., device_results=True)`` returns: the detections of the whole run in device memory.
    ``rows``: ONE float32 tensor [N, M, W] -- N samples in dataset order, M = ``test_cfg.max_per_img`` rows each, W = 7 + 3K
    columns in the layout of ``get_bboxes_packed_tensor`` (box, score, label, count, landmarks); rows at or beyond a sample's
    count hold nothing and are never read.  ``evaluation_device.evaluate_results`` packs it where it lies
    (``pack_device_results``).  ``to_host()``: the list the plain ``single_gpu_test`` returns, array for array (what ``--out``
    pickles take); ``release()`` drops ``rows``.  ``num_classes``: the head's (labels are 0 .. num_classes - 2)."""

    def __init__(self, rows, num_classes, unpack=None):
        self.rows, self.num_classes, self._unpack = rows, int(num_classes), unpack

    def __len__(self):
        return 0 if self.rows is None else int(self.rows.shape[0])

    def to_host(self):
        if self.rows is None:
            raise ValueError('the device results were released')
        from .detector import RepPointsDetectorKp
        unpack = self._unpack
        if unpack is None:
            from .decode import unpack_results as unpack
        # (bbox2result_kp reads nothing of its detector -- it is called without one here; it has to stay that way)
        return [RepPointsDetectorKp.bbox2result_kp(None, d.copy(), lab, k, self.num_classes)
                for d, lab, k in unpack(self.rows.cpu().numpy())]

    def release(self):
        self.rows = None


class _RowSink(object):
    """where ``_test_on`` / ``_test_on_device`` leave their detections for ``device_results``: every group's packed block is
    copied into its slice of ONE [n, M, W] tensor on the device (allocated at the first block), no download"""

    def __init__(self, n):
        self.n, self.at, self.rows = n, 0, None

    def put(self, block):
        if self.rows is None:
            self.rows = torch.empty((self.n,) + tuple(block.shape[1:]), dtype=torch.float32, device=block.device)
        self.rows[self.at:self.at + block.shape[0]].copy_(block)
        self.at += block.shape[0]

    def single(self, model, imgs, metas, rescale):
        """one sample, as ``forward_test`` dispatches it: one augmentation or test-time augmentation"""
        target = model.module if hasattr(model, 'module') else model
        if len(imgs) != len(metas):
            raise ValueError('num of augmentations ({}) != num of image meta ({})'.format(len(imgs), len(metas)))
        assert imgs[0].size(0) == 1
        if len(imgs) == 1:
            self.put(target.simple_test_batch_device(imgs[0], metas[0], rescale=rescale))
        else:
            self.put(target.aug_test_device(imgs, metas, rescale=rescale))

    def batch(self, model, img, metas, rescale):
        self.put(model.simple_test_batch_device(img, metas, rescale=rescale))


class _Prefetched(object):
    """``fn(indices[k])`` for k = 0, 1, 2, ... as the test loops ask for them -- strictly in that order, each once --, computed in
    a pool of ``workers`` threads (at most 16) a bounded window ahead (two samples per thread).  Test-time samples make no
    random draws, so the whole preparation runs in the pool; an exception there is raised by the call that asks for its
    sample, with its type."""

    def __init__(self, fn, indices, workers):
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        workers = min(int(workers), 16)
        self.fn, self.indices, self.window = fn, indices, 2 * workers
        self.pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix='kgdet-test-prefetch')
        self.futures, self.at, self.submitted = deque(), 0, 0

    def __call__(self, k):
        assert k == self.at, 'the test loops read their samples in order, each once'
        while self.submitted < min(len(self.indices), k + 1 + self.window):
            self.futures.append(self.pool.submit(self.fn, self.indices[self.submitted]))
            self.submitted += 1
        self.at += 1
        return self.futures.popleft().result()

    def close(self):
        self.pool.shutdown(wait=True, cancel_futures=True)


def _test_on(model, dataset, indices, rescale, to_device, imgs_per_gpu=1, device_preprocess=False, sink=None, workers=0,
             show=None, device_decode=False):
    """results of the samples ``indices`` in that order.  imgs_per_gpu == 1: the reference's call, one image per forward
    (``model(return_loss=False, rescale=..., **data)``, tools/test.py:25-28); > 1: runs of consecutive samples with identical
    tensor shapes and one augmentation go through ``simple_test_batch`` together (the same per-image results: nothing in
    backbone / neck / head / decode / NMS mixes the images of a batch).  ``device_preprocess``: the input transform runs on the
    model's GPU from the raw pixels (``_test_on_device``; ``to_device`` is not used then).  ``workers`` > 0: the samples are
    prepared ahead in that many threads (``_Prefetched``) and consumed in the same order -- the same calls, the same results.
    ``show``: a ``_Show`` that draws every group's images once its detections exist.  ``device_decode`` (with
    ``device_preprocess``): the samples carry their FILES (``dataset.load_image_file``; the threads only read and parse headers)
    and every group is decoded on the GPU in one call (``jpeg.DeviceDecodeRoute``) -- the same pixels, the same results; True
    or 'camera' (4:2:2 files and restart intervals as well, ``jpeg.parse_header(camera=True)``)."""
    if workers < 0:
        raise ValueError('workers is >= 0, got %r' % (workers,))
    if device_decode and not device_preprocess:
        raise ValueError('device_decode=True needs device_preprocess=True: the decoded images stay on the GPU')
    prepare = None
    from .jpeg import decode_switch
    device_decode, camera = decode_switch(device_decode)       # (True or 'camera', which also takes 4:2:2 and DRI files)
    if device_decode:
        def prepare(idx):
            return dataset.prepare_test_raw(idx, img=dataset.load_image_file(idx, camera=True) if camera else dataset.load_image_file(idx))
    if workers:
        fn = (prepare or dataset.prepare_test_raw) if device_preprocess else dataset.__getitem__
        ahead = _Prefetched(fn, indices, workers)
        try:
            return _test_loop(model, dataset, indices, rescale, to_device, imgs_per_gpu, device_preprocess, sink, ahead, show, prepare, camera)
        finally:
            ahead.close()
    return _test_loop(model, dataset, indices, rescale, to_device, imgs_per_gpu, device_preprocess, sink, None, show, prepare, camera)


def _test_loop(model, dataset, indices, rescale, to_device, imgs_per_gpu, device_preprocess, sink, ahead, show=None, prepare=None,
               camera=False):
    if device_preprocess:
        return _test_on_device(model, dataset, indices, rescale, imgs_per_gpu, sink, ahead, show, prepare, camera)
    model.eval()
    results, i = [], 0
    carried = None                 # the sample that ended the previous group (loaded once)
    while i < len(indices):
        data = carried if carried is not None else (dataset[indices[i]] if ahead is None else ahead(i))
        carried = None
        group = [data]
        while (imgs_per_gpu > 1 and len(group) < imgs_per_gpu and i + len(group) < len(indices) and len(data['img']) == 1):
            nxt = dataset[indices[i + len(group)]] if ahead is None else ahead(i + len(group))
            if len(nxt['img']) != 1 or nxt['img'][0].shape != data['img'][0].shape:
                carried = nxt
                break
            group.append(nxt)
        with torch.no_grad():
            if len(group) == 1:
                imgs = [t[None] for t in data['img']]
                metas = [[m] for m in data['img_meta']]
                if to_device is not None:
                    imgs = [to_device(t) for t in imgs]
                if sink is not None:
                    sink.single(model, imgs, metas, rescale)
                else:
                    results.append(model(imgs, metas, return_loss=False, rescale=rescale))
            else:
                img = torch.stack([g['img'][0] for g in group])
                if to_device is not None:
                    img = to_device(img)
                if sink is not None:
                    sink.batch(model, img, [g['img_meta'][0] for g in group], rescale)
                else:
                    results.extend(model.simple_test_batch(img, [g['img_meta'][0] for g in group], rescale=rescale))
        if show is not None:
            show.group(indices[i:i + len(group)], None, results, sink)
        i += len(group)
    return results


def _test_on_device(model, dataset, indices, rescale, imgs_per_gpu=1, sink=None, ahead=None, show=None, prepare=None, camera=False):
    """``_test_on`` with the input transform on the GPU: samples come from ``dataset.prepare_test_raw`` (raw uint8 pixels +
    planned metas) and go through ``preprocess.DeviceImageTransform`` on the model's device -- one launch per group of
    ``imgs_per_gpu`` single-augmentation samples with the same planned ``pad_shape`` (the grouping of ``_test_on``, whose
    tensor shapes ARE the pad shapes), one launch for all augmentations of a TTA sample (its raw image uploaded once).
    ``prepare``: the ``device_decode`` route's ``prepare_test_raw``, whose ``raw`` is the image's file: the group's files are
    decoded in one call before the transform (``camera``: by ``kgdet_jpeg_decode_camera``, for files ``prepare`` parsed with that switch)."""
    model.eval()
    device = next(model.parameters()).device
    transform = dataset.device_transform(device)
    route = None
    if prepare is not None:
        from .jpeg import DeviceDecodeRoute
        route = DeviceDecodeRoute(device, camera)
    prepare = prepare or dataset.prepare_test_raw
    results, i = [], 0
    carried = None
    while i < len(indices):
        data = carried if carried is not None else (prepare(indices[i]) if ahead is None else ahead(i))
        carried = None
        group = [data]
        while (imgs_per_gpu > 1 and len(group) < imgs_per_gpu and i + len(group) < len(indices)
               and len(data['img_meta']) == 1):
            nxt = prepare(indices[i + len(group)]) if ahead is None else ahead(i + len(group))
            if len(nxt['img_meta']) != 1 or nxt['img_meta'][0]['pad_shape'] != data['img_meta'][0]['pad_shape']:
                carried = nxt
                break
            group.append(nxt)
        if route is not None:
            group = [dict(g, raw=r) for g, r in zip(group, route([g['raw'] for g in group]))]
            data = group[0]
        with torch.no_grad():
            if len(group) == 1:
                imgs, _ = transform.separate([data['raw']] * len(data['scales']), data['scales'], data['flips'],
                                             keep_ratio=data['keep_ratio'])
                if sink is not None:
                    sink.single(model, imgs, [[m] for m in data['img_meta']], rescale)
                else:
                    results.append(model(imgs, [[m] for m in data['img_meta']], return_loss=False, rescale=rescale))
            else:
                img, _ = transform([g['raw'] for g in group], [g['scales'][0] for g in group],
                                   [g['flips'][0] for g in group], keep_ratio=data['keep_ratio'])
                if sink is not None:
                    sink.batch(model, img, [g['img_meta'][0] for g in group], rescale)
                else:
                    results.extend(model.simple_test_batch(img, [g['img_meta'][0] for g in group], rescale=rescale))
        if show is not None:
            show.group(indices[i:i + len(group)], [g['raw'] for g in group], results, sink)
        i += len(group)
    return results


class _Show(object):
    """``single_gpu_test(..., show_dir=...)``: once a group's detections exist, its original-size images -- ``raws``, or
    ``dataset.load_image`` -- are drawn in one launch (``visualize.DeviceDrawer``) from the group's rows: the slice of the
    sink's device tensor with ``device_results``, else the results just computed, packed and uploaded.  Only the finished
    pictures come back to the host, where ``visualize.PictureWriter``'s threads encode them into
    ``show_dir/<basename of the image file><ext>``.  ``encoder='device'``: the drawn group stays where it is, is encoded there
    (``jpeg.DeviceJpegEncoder``, quality 90), only the files' bytes come down and the threads only write them."""

    def __init__(self, model, dataset, show_dir, score_thr, ext, workers, encoder='host'):
        from .visualize import PictureWriter
        if encoder not in ('host', 'device'):
            raise ValueError("show_encoder is 'host' or 'device', got %r" % (encoder,))
        if encoder == 'device' and ext.lower() not in ('.jpg', '.jpeg'):
            raise ValueError("show_encoder='device' writes JPEG files: show_ext is .jpg, got %r" % (ext,))
        self.encoder = None
        target = model.module if hasattr(model, 'module') else model
        self.dataset, self.score_thr = dataset, score_thr
        self.device = next(target.parameters()).device
        L = target.bbox_head.num_classes - 1
        names = list(getattr(target, 'CLASSES', None) or getattr(dataset, 'CLASSES', None) or [])
        self.names = names if len(names) == L else ['%d' % c for c in range(L)]
        self.drawers = {}                     # by K: an image without detections comes as rows of one landmark
        self.writer = PictureWriter(show_dir, workers, ext)
        if encoder == 'device':
            from .jpeg import DeviceJpegEncoder
            self.encoder = DeviceJpegEncoder(90, device=self.device)

    def name(self, idx):
        filename = self.dataset.img_infos[idx].get('filename')
        return os.path.basename(filename) if filename else 'image_%06d' % idx

    def group(self, idxs, raws, results, sink):
        from .visualize import DeviceDrawer, default_ranges, stack_result_rows
        n = len(idxs)
        block = stack_result_rows(results[-n:]) if sink is None else sink.rows[sink.at - n:sink.at]
        K = (block.shape[2] - 7) // 3
        if K not in self.drawers:
            self.drawers[K] = DeviceDrawer(self.names, landmark_ranges=default_ranges(len(self.names), K), score_thr=self.score_thr,
                                           device=self.device)
        if raws is None:
            raws = [self.dataset.load_image(i) for i in idxs]
        if self.encoder is not None:
            for idx, data in zip(idxs, self.encoder(self.drawers[K](raws, block, to_host=False))):
                self.writer.put_bytes(data, self.name(idx))
            return
        for idx, picture in zip(idxs, self.drawers[K](raws, block, to_host=True)):
            self.writer.put(picture, self.name(idx))

    def close(self, failed=False):
        self.writer.close(failed)


def single_gpu_test(model, dataset, rescale=True, to_device=None, imgs_per_gpu=1, device_preprocess=False,
                    device_results=False, workers=0, show_dir=None, show_score_thr=0.3, show_ext='.jpg', show_encoder='host',
                    device_decode=False):
    """tools/test.py:18-35 without the progress bar: one result per sample, in dataset order.  ``device_preprocess``:
    resize / normalise / flip / pad on the model's GPU from the raw pixels (``_test_on_device``; ``to_device`` is not
    used then) instead of ``dataset[i]``'s host transform; same result format and order.  ``device_results``: the
    detections stay on the device -- a ``DeviceResults`` comes back instead of the list (its ``to_host()`` IS that list): no
    download and no per-class split per batch.  ``NotImplementedError`` for ``test_cfg.max_per_img <= 0`` (before the run) or
    an image with more detections than that.  ``workers``: threads that decode and prepare the upcoming samples (``_test_on``);
    0 prepares each sample inline, as the reference's loop does.  ``show_dir`` (the reference's ``--show``, into files): every
    image is drawn at its original size with the detections above ``show_score_thr`` (``_Show``) and written to
    ``show_dir/<basename of the image file><show_ext>`` ('.jpg' at quality 90, or '.png') by ``workers`` threads, at least 1, at
    most 16; what the call returns does not change.  It needs ``rescale=True`` (``ValueError`` before the run); a writer's
    exception is re-raised, and the threads are gone when the call returns or raises.  ``show_encoder``: 'host' -- the drawn
    pictures are downloaded and the threads encode them (PIL); 'device' -- they are encoded on the GPU (``jpeg.py``: baseline
    JPEG, quality 90, the bytes of ``jpeg.jpeg_restatement``, not PIL's), only the files come down and the threads only write;
    it takes ``show_ext`` '.jpg' / '.jpeg' (``ValueError`` before the run).  ``device_decode``: the JPEG files are decoded on
    the GPU as well (``jpeg.DeviceDecodeRoute``: every group of the loop in one call, ``workers`` then only read files); it
    needs ``device_preprocess=True`` (``ValueError`` before the run); same results.  True, or 'camera': 4:2:2 files and files
    with restart intervals are decoded on the device too instead of by PIL with a warning."""
    if device_decode and not device_preprocess:
        raise ValueError('device_decode=True needs device_preprocess=True: the decoded images stay on the GPU')
    if show_dir is None:
        return _single_gpu_test(model, dataset, rescale, to_device, imgs_per_gpu, device_preprocess, device_results, workers, None,
                                device_decode)
    if not rescale:
        raise ValueError('show_dir draws on the original images: it needs rescale=True')
    show = _Show(model, dataset, show_dir, show_score_thr, show_ext, workers, show_encoder)
    failed = True
    try:
        out = _single_gpu_test(model, dataset, rescale, to_device, imgs_per_gpu, device_preprocess, device_results, workers, show,
                               device_decode)
        failed = False
    finally:
        show.close(failed)
    return out


def _single_gpu_test(model, dataset, rescale, to_device, imgs_per_gpu, device_preprocess, device_results, workers, show,
                     device_decode=False):
    if not device_results:
        return _test_on(model, dataset, list(range(len(dataset))), rescale, to_device, imgs_per_gpu, device_preprocess,
                        workers=workers, show=show, device_decode=device_decode)
    target = model.module if hasattr(model, 'module') else model
    M = int(target.test_cfg.max_per_img)
    if M <= 0:
        raise NotImplementedError('device results need test_cfg.max_per_img > 0 (the rows per image)')
    sink = _RowSink(len(dataset))
    _test_on(model, dataset, list(range(len(dataset))), rescale, to_device, imgs_per_gpu, device_preprocess, sink, workers, show,
             device_decode)
    rows = sink.rows
    if rows is None:                            # (an empty dataset)
        rows = torch.empty((0, M, 10), dtype=torch.float32, device=next(target.parameters()).device)
    assert sink.at == len(dataset)
    return DeviceResults(rows, target.bbox_head.num_classes, getattr(target.bbox_head, 'unpack_results', None))


def collect_results(result_part, size, group=None):
    """tools/test.py:61-100 with the gather done by the process group instead of pickles in a shared temporary directory:
    rank 0 receives every rank's list, interleaves them (sample k of rank r is dataset index k * world_size + r), cuts the
    padding samples off and returns ``size`` results; the other ranks return None."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return list(result_part)[:size]
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    parts = [None] * world if rank == 0 else None
    dist.gather_object(result_part, parts, dst=0, group=group)
    if rank != 0:
        return None
    if len(set(len(p) for p in parts)) != 1:
        raise RuntimeError('ranks returned different numbers of results: %s (the shards of test_shard are equally long)'
                           % [len(p) for p in parts])
    ordered = []
    for res in zip(*parts):          # (every rank holds the same number of samples: the index list was padded)
        ordered.extend(list(res))
    return ordered[:size]


def multi_gpu_test(model, dataset, rescale=True, to_device=None, imgs_per_gpu=1, group=None, device_preprocess=False,
                   workers=0):
    """tools/test.py:38-58: every rank runs its shard of the dataset, rank 0 returns all results in dataset order
    (``device_preprocess`` and ``workers``: as in ``single_gpu_test``, on each rank's own device)"""
    import torch.distributed as dist
    on = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if on else 1
    rank = dist.get_rank(group) if on else 0
    part = _test_on(model, dataset, test_shard(len(dataset), world, rank), rescale, to_device, imgs_per_gpu,
                    device_preprocess, workers=workers)
    return collect_results(part, len(dataset), group)


class GraphedTrainStep(object):
    """One training step of a FIXED-shape batch -- forward, the nine losses, backward, gradient clip, Adam or momentum SGD (the
    project's fused steps, or torch's fused SGD when the optimizer was built with ``fused=True``: config 5) -- as ONE HIP graph.

    The eager step is ~560 kernel launches whose enqueue (Python module calls + launch latency, ~11 ms at full size) takes as
    long as the GPU needs to run them (``tools/host_step_cost.py``): every kernel gain below a few percent is invisible in
    images/s.  Nothing in the step reads back to the host (``tests/test_gpu_head.py::test_training_step_has_no_host_syncs``), the
    optimizer's schedule lives in device memory (``optim.FusedClipAdam.enable_device_schedule``: step count, bias corrections
    and the learning rate are not kernel arguments; ``optim.FusedClipSGD`` likewise with the learning rate alone, so a plain
    ``torch.optim.SGD`` as ``build_optimizer`` makes it from the DeepFashion2 configs is captured too), so the whole step is
    captured once (``torch.cuda.CUDAGraph`` = hipGraph)
    and replayed per iteration.  The reference has no equivalent (``mmdet/apis/train.py:17-134`` + mmcv's Runner issue every
    op eagerly); the arithmetic is the eager step's, kernel by kernel.

    ``batch``: the dict ``forward_train`` takes (``img`` [B, 3, H, W], ``img_meta``, ``gt_bboxes`` / ``gt_labels`` /
    ``gt_keypoints`` lists of CUDA tensors): these tensors become the graph's input buffers; ``load(batch)`` copies another
    batch of the SAME shapes (same number of ground-truth rows per image) into them, ``step()`` publishes the step's learning
    rate (``optimizer.param_groups[0]['lr']``, as set by ``LrSchedule``), replays the graph and returns the loss tensors of
    the step (device tensors, overwritten by the next replay).  One rank only: the gradient exchange of a multi-rank job
    stays on the eager path (``DistOptimizerHook``).  ``sync_optimizer_state()`` before the optimizer's state is read
    (checkpoints): the replayed steps are added to its ``step`` counters then."""

    def __init__(self, model, optimizer, opt_hook, batch, warmup=3, batch_processor=batch_processor):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError('the graphed step covers one rank; a multi-rank job exchanges gradients eagerly')
        from .optim import FusedClipAdam, FusedClipSGD
        self.model, self.optimizer, self.hook = model, optimizer, opt_hook
        self.static = batch
        self._rebuild = dict(warmup=warmup, batch_processor=batch_processor)
        self.static_tensors = [batch['img']] + [t for k in ('gt_bboxes', 'gt_labels', 'gt_keypoints') for t in batch.get(k, [])]
        assert all(t.is_cuda for t in self.static_tensors) and model.training

        def one_step():
            if getattr(self, 'lr_t', None) is not None and torch.cuda.is_current_stream_capturing():
                self.lr_t.copy_(self.lr_pin[0], non_blocking=True)
            out = batch_processor(model, self.static, train_mode=True)
            opt_hook.step(model, optimizer, out['loss'])
            return out

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(int(warmup), 2)):      # optimizer state, weight-image sets, MIOpen find: all before the capture
                one_step()
        torch.cuda.current_stream().wait_stream(side)
        fused, fused_sgd = opt_hook._fused, getattr(opt_hook, '_fused_sgd', None)
        self.fused, self.lr_t = None, None
        if fused is not None and len(optimizer.param_groups) == 1 and \
                FusedClipAdam.applicable(optimizer, opt_hook._params, opt_hook.grad_clip):
            if fused._sched is None:
                fused.enable_device_schedule(optimizer)
            self.fused = fused
        elif fused_sgd is not None and FusedClipSGD.applicable(optimizer, opt_hook._params, opt_hook.grad_clip):
            # plain torch.optim.SGD (the DeepFashion2 configs): the project's clip + SGD step with the rate in device memory, fed
            # through the page-locked ring -- a rate change (every step of the warm-up) costs no synchronisation
            if fused_sgd._sched is None:
                fused_sgd.enable_device_schedule(optimizer)
            self.fused = fused_sgd
        elif (type(optimizer) is torch.optim.SGD and len(optimizer.param_groups) == 1
              and optimizer.param_groups[0].get('fused') and not optimizer.param_groups[0].get('nesterov')):
            # torch's fused SGD (config 5: momentum 0.9, weight decay 1e-4) keeps no step count; with the learning rate as a
            # DEVICE scalar the whole step -- clip_grad_norm_'s foreach chain included -- is capturable: `step()` writes the
            # scheduler's rate into that scalar before every replay (a fill kernel, no read-back)
            group = optimizer.param_groups[0]
            self.lr_t = torch.tensor(float(group['lr']), dtype=torch.float32, device=self.static_tensors[0].device)
            # the rate reaches the device scalar through a copy node at the head of the graph, from ONE page-locked host scalar that
            # `step()` rewrites only when the scheduler's value changed (after waiting for the replays that still read the old one)
            self.lr_pin = torch.tensor([float(group['lr'])], dtype=torch.float32).pin_memory()
            self._lr_last = float(group['lr'])
        else:
            raise NotImplementedError('the graphed step needs the fused clip + Adam step, the fused clip + SGD step (a plain '
                                      'torch.optim.SGD on CUDA fp32 parameters) or torch.optim.SGD(fused=True) without Nesterov '
                                      'momentum -- one parameter group in every case')
        group = optimizer.param_groups[0]
        lr_host = group['lr']
        if self.lr_t is not None:
            group['lr'] = self.lr_t
        try:
            with torch.cuda.stream(side):                  # one eager step in the captured form (its table, its buffers)
                one_step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            optimizer.zero_grad(set_to_none=True)
            if self.fused is not None:
                self.fused.publish_lr(optimizer)
            with torch.cuda.graph(self.graph):
                self.out = one_step()
        finally:
            if self.lr_t is not None:
                group['lr'] = lr_host                      # (schedulers keep seeing and setting a float)
        # (the capture itself does not run the step: nothing was counted yet)
        self.steps = 0
        # the captured launches hold each convolution's operand format and the pack table's address: conv1x1.set_bf16_parts refuses
        # to change a route of this model until `retire()`
        from . import conv1x1
        conv1x1.register_capture(self)

    def retire(self):
        """give the graph up (its launches bake in the operand formats and table addresses of the capture): after this the routes
        of the model's convolutions may change (conv1x1.set_bf16_parts); ``recapture()`` builds the step again"""
        from . import conv1x1
        torch.cuda.synchronize()
        conv1x1.release_capture(self)
        self.graph = self.out = None

    def recapture(self):
        """a new GraphedTrainStep of the same model, optimizer, hook and input buffers (like the first capture it takes warm-up
        steps on the batch in the buffers); the steps counted so far carry over"""
        if self.graph is not None:
            self.retire()
        new = GraphedTrainStep(self.model, self.optimizer, self.hook, self.static, **self._rebuild)
        new.steps = self.steps
        return new

    def load(self, batch):
        new = [batch['img']] + [t for k in ('gt_bboxes', 'gt_labels', 'gt_keypoints') for t in batch.get(k, [])]
        if len(new) != len(self.static_tensors) or any(a.shape != b.shape for a, b in zip(new, self.static_tensors)):
            raise ValueError('the graphed step was captured for other tensor shapes')
        if self.lr_t is not None or type(self.optimizer) is torch.optim.SGD:
            # (every SGD optimizer, whichever step it takes)
            # Observed on this stack (ROCm 7.0 / torch 2.10, tools/graph_serial_probe.py): an eager kernel enqueued BEHIND an in-flight
            # replay of the config-5 (serial head, SGD) graph ends in an HSA hardware exception (0x1016) -- the KGDet graph takes the
            # same pattern without complaint (tools/graph_load_probe.py), a replay that has finished is fine in both.  Cause not
            # found; until it is, this flow waits for the replay before it touches the graph's input buffers.
            torch.cuda.current_stream().synchronize()
        with torch.no_grad():
            torch._foreach_copy_(self.static_tensors, [t.to(s.device, non_blocking=True) for t, s in zip(new, self.static_tensors)])

    def step(self):
        if self.fused is not None:
            self.fused.publish_lr(self.optimizer)
            self.graph.replay()
            self.fused.step_published()
        else:
            lr = float(self.optimizer.param_groups[0]['lr'])
            if lr != self._lr_last:
                torch.cuda.current_stream().synchronize()     # (replays in flight read the scalar's old value)
                self.lr_pin[0] = lr
                self._lr_last = lr
            self.graph.replay()
        self.steps += 1
        # the replayed kernels wrote the parameters through raw pointers: the version counters did not move, and the inference-time
        # copies derived from the weights (conv1x1._cast_cache, the folded backbone, the packed deformable operands) are keyed on them
        self._stale_caches = True
        return self.out

    def refresh_inference_caches(self):
        """after replays, before an evaluation pass of the same model: drops every derived copy of the stepped weights (also done
        by ``model.eval()`` / ``model.train()`` of the detector, detector.py)"""
        if getattr(self, '_stale_caches', False):
            from . import conv1x1
            conv1x1.invalidate_inference_caches()
            self._stale_caches = False

    def sync_optimizer_state(self):
        if self.fused is not None:
            self.fused.sync_optimizer_state(self.optimizer)


class Runner(object):
    def __init__(self, model, optimizer, work_dir=None, lr_config=None, optimizer_config=None, checkpoint_config=None,
                 log_interval=50, logger=print, batch_processor=batch_processor, eval_config=None, on_record=None):
        """``eval_config = dict(dataset=..., interval=1, imgs_per_gpu=1, device_preprocess=False, group=None, to_device=None,
        result_types=('bbox', 'keypoints'), device=None, lazy_landmarks=None, device_accumulate=None, device_results=False,
        workers=0, device_decode=False)``:
        validation after every ``interval``-th epoch (``validate``); ``lazy_landmarks`` and ``device_accumulate`` are
        ``evaluation_device.evaluate_results``'s, ``device_results``, ``workers`` and ``device_decode`` are ``single_gpu_test``'s (``device_results``
        and ``device_decode`` with ``group`` are refused: ``multi_gpu_test`` gathers host lists).  ``on_record(mode, record)``: called with 'train' or
        'val' and every record as it is appended to ``log_history`` (``apis.train_detector`` writes its ``.log.json`` there)."""
        self.model, self.optimizer, self.work_dir = model, optimizer, work_dir
        self.eval_config = dict(eval_config) if eval_config else None
        if self.eval_config and self.eval_config.get('device_results') and self.eval_config.get('group') is not None:
            raise ValueError('eval_config: device_results covers single_gpu_test only, not a process group')
        if self.eval_config and self.eval_config.get('device_decode') and self.eval_config.get('group') is not None:
            raise ValueError('eval_config: device_decode covers single_gpu_test only, not a process group')
        self._packed_gt = None
        self.lr = LrSchedule(**(lr_config or dict(policy='step', step=[])))
        self.opt_hook = DistOptimizerHook(**(optimizer_config or {}))
        self.ckpt_interval = (checkpoint_config or {}).get('interval', 1)
        self.log_interval, self.logger, self.batch_processor = log_interval, logger, batch_processor
        self.epoch, self.iter = 0, 0
        self.log_history, self.on_record = [], on_record
        self.graphed = None      # a GraphedTrainStep driven by the caller (`attach_graphed`): re-captured when a layer is rerouted

    def attach_graphed(self, step):
        """tell the runner about the GraphedTrainStep the caller replays between its epochs: `check_envelope` builds it again when
        it has to change a convolution's operand format (read ``runner.graphed`` afterwards)"""
        self.graphed = step
        return step

    def check_envelope(self):
        """The envelope of the fp16-part convolutions (numerics.py) on the model's current weights, policy ``KGDET_ENVELOPE``: run
        at the end of every epoch, before validation and the checkpoint write -- one scan launch and one read-back, nothing inside
        the step.  CUDA models only.  A reroute underneath a graphed step retires the step first and captures it again.
        -> the violations that led to a reroute"""
        target = self.model.module if hasattr(self.model, 'module') else self.model
        if os.environ.get('KGDET_ENVELOPE', 'bf16') == 'off' or not any(p.is_cuda for p in target.parameters()):
            return []
        from . import numerics
        retired = []

        def before_reroute():
            if self.graphed is not None and self.graphed.graph is not None:
                self.graphed.retire()
                retired.append(self.graphed)

        _, rerouted = numerics.enforce(target, before_reroute=before_reroute)
        if retired:
            self.graphed = retired[0].recapture()
            self.logger('envelope: %d layer(s) rerouted to bf16 parts, the graphed step was captured again' % len(rerouted))
        return rerouted

    def _record(self, mode, rec):
        self.log_history.append(rec)
        if self.on_record is not None:
            self.on_record(mode, rec)

    def current_lr(self):
        return [g['lr'] for g in self.optimizer.param_groups]

    def save_checkpoint(self, filename_tmpl='epoch_{}.pth', create_latest=True):
        path = os.path.join(self.work_dir, filename_tmpl.format(self.epoch))
        save_checkpoint(self.model, path, optimizer=self.optimizer, meta=dict(epoch=self.epoch, iter=self.iter))
        if create_latest:
            shutil.copyfile(path, os.path.join(self.work_dir, 'latest.pth'))
        return path

    def resume(self, checkpoint, resume_optimizer=True, map_location='cpu'):
        ckpt = load_checkpoint(self.model, checkpoint, map_location=map_location)
        self.epoch, self.iter = ckpt['meta']['epoch'], ckpt['meta']['iter']
        if 'optimizer' in ckpt and resume_optimizer:
            self.optimizer.load_state_dict(ckpt['optimizer'])
        self.logger('resumed epoch %d, iter %d' % (self.epoch, self.iter))
        return ckpt

    def train_epoch(self, data_loader, to_device=None):
        """``to_device(data)`` turns what the loader yields into the batch dict on the GPU.  For the device-side input
        transform let the loader yield lists of ``dataset.prepare_train_raw`` samples and pass
        ``to_device=lambda samples: move(datasets.collate_device(samples, dataset.device_transform()))`` with ``move``
        the usual host->device copy of the ground-truth lists (the image is made on the GPU by one launch) -- or hand in a
        ``loader.build_dataloader(..., device=...)``, whose batches are on the GPU already (``to_device=None``).  Each log record
        carries ``data_time`` beside ``time``: the mean seconds per iteration spent waiting in the loader's ``next()`` (mmcv's field
        of that name) -- the number that says whether the feed keeps up."""
        self.model.train()
        self.lr.before_train_epoch(self.optimizer, self.epoch)
        t0, waited = time.time(), 0.0
        batches, i = iter(data_loader), -1
        while True:
            t_next = time.time()
            try:
                data = next(batches)
            except StopIteration:
                break
            waited += time.time() - t_next
            i += 1
            self.lr.before_train_iter(self.optimizer, self.iter)
            if to_device is not None:
                data = to_device(data)
            out = self.batch_processor(self.model, data, train_mode=True)
            self.opt_hook.step(self.model, self.optimizer, out['loss'])
            self.iter += 1
            if self.log_interval and (i + 1) % self.log_interval == 0:
                rec = OrderedDict(epoch=self.epoch + 1, iter=i + 1, lr=self.current_lr()[0],
                                  time=(time.time() - t0) / (i + 1), data_time=waited / (i + 1))
                rec.update((k, float(v.detach()) if isinstance(v, torch.Tensor) else float(v)) for k, v in out['log_vars'].items())     # the only device->host read
                self._record('train', rec)
                self.logger(', '.join('%s: %.5g' % kv if isinstance(kv[1], float) else '%s: %s' % kv for kv in rec.items()))
        self.epoch += 1

    def run(self, data_loader, max_epochs, to_device=None, set_epoch=None):
        self.lr.before_run(self.optimizer)
        while self.epoch < max_epochs:
            if set_epoch is not None:
                set_epoch(self.epoch)
            self.train_epoch(data_loader, to_device)
            self.check_envelope()
            if self.work_dir is not None and self.ckpt_interval > 0 and self.epoch % self.ckpt_interval == 0:
                self.save_checkpoint()
            if self.eval_config is not None and self.epoch % self.eval_config.get('interval', 1) == 0:
                self.validate()
        return self

    def validate(self):
        """The reference's ``CocoDistEvalmAPHook`` (mmdet/core/evaluation/eval_hooks.py:136-172) after a training epoch: the
        model in ``eval()``, ``single_gpu_test`` -- ``multi_gpu_test`` when ``eval_config['group']`` is given -- over the
        validation dataset, the results evaluated on rank 0 without result files (``evaluation_device.evaluate_results``, on
        the GPU unless ``eval_config['device']`` says otherwise), one record appended to ``log_history`` and logged, the model
        back in ``train()`` (which drops the inference-time weight caches).  The ground truth is packed once and kept.
        Record: ``epoch`` and, per result type, ``{type}_mAP``, ``_mAP_50``, ``_mAP_75``, ``_mAP_s``, ``_mAP_m``, ``_mAP_l`` =
        ``float('%.3f' % stats[i])`` for i = 0..5 plus ``{type}_mAP_copypaste``.  As in the reference the six names are applied
        to ``stats[0..5]`` of EITHER type: for 'keypoints' ``stats[3..5]`` are AP-medium, AP-large and AR, not small / medium /
        large.  Callers of ``GraphedTrainStep`` run ``refresh_inference_caches()`` and then this method between replays.
        Returns the record (None on the other ranks)."""
        from . import evaluation_device as evd
        cfg = self.eval_config
        dataset, group = cfg['dataset'], cfg.get('group')
        was_training = self.model.training
        self.model.eval()
        try:
            kw = dict(rescale=True, to_device=cfg.get('to_device'), imgs_per_gpu=cfg.get('imgs_per_gpu', 1),
                      device_preprocess=cfg.get('device_preprocess', False), workers=cfg.get('workers', 0))
            if group is not None:
                results = multi_gpu_test(self.model, dataset, group=group, **kw)
            else:
                results = single_gpu_test(self.model, dataset, device_results=bool(cfg.get('device_results', False)),
                                          device_decode=cfg.get('device_decode', False), **kw)
        finally:
            self.model.train(was_training)
        if results is None:                     # (not rank 0)
            return None
        if self._packed_gt is None:
            self._packed_gt = evd.pack_ground_truth(dataset.coco)
        device = cfg.get('device')
        if device is None:
            device = next(self.model.parameters()).device
        types = [t for t in cfg.get('result_types', ('bbox', 'keypoints'))
                 if t == 'bbox' or isinstance(results, DeviceResults) or isinstance(results[0], tuple)]
        stats = evd.evaluate_results(dataset, results, types, device=device, packed_gt=self._packed_gt,
                                     lazy_landmarks=cfg.get('lazy_landmarks'), device_accumulate=cfg.get('device_accumulate'))
        rec = OrderedDict(epoch=self.epoch)
        for t in types:
            names = ['mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l']
            for i, name in enumerate(names):
                rec['{}_{}'.format(t, name)] = float('{:.3f}'.format(stats[t][i]))
            rec['{}_mAP_copypaste'.format(t)] = ('{:.3f} ' * 6).format(*stats[t][:6]).strip()
        self._record('val', rec)
        self.logger(', '.join('%s: %s' % kv for kv in rec.items()))
        return rec
