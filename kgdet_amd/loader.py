"""The training feed: ``build_dataloader`` (``mmdet/datasets/loader/build_loader.py:17-48``) on threads.

The reference hands the dataset to ``torch.utils.data.DataLoader`` with worker PROCESSES.  Here the only expensive host
work per sample is the JPEG decode, and PIL releases the GIL while it decodes, so a pool of threads buys the same
parallelism without a second GPU context, without pickling samples and with one RNG stream.

Pipeline per sample (``workers_per_gpu > 0``)::

    decode   dataset.load_image(idx)                       pool, ahead of use, in the epoch's known index order
    draws    dataset.prepare_train_raw(idx, img=decoded)   ONE thread, in sampler order (numpy's global RNG)
    pixels   datasets.finish_train_sample(dataset, raw)    pool (host route only)
    batch    collate / ground-truth packing                pool, into page-locked memory when ``device`` is given
    upload   one non-blocking copy, ``collate_device``     the consuming thread, inside ``__next__``

Determinism contract.  For one seed of numpy's global RNG the loader yields, for ANY ``workers_per_gpu`` and ``prefetch``,
exactly the batches of the serial loop -- ``order = list(sampler)`` and then, batch by batch,
``collate([dataset[i] for i in ...])`` (``prepare_train_raw`` with ``__getitem__``'s resample for the raw route) -- and
leaves that RNG in the same state after the epoch.  The resample of an image without annotations (an extra
``np.random.choice`` on ``dataset.flag`` and a decode nobody prefetched) is made by the drawing thread at the sample's place in
the order, as in the serial loop.  The loader OWNS numpy's global RNG while an epoch is in flight: the draws run up to
``prefetch`` batches ahead of the consumer, so a program that draws from it elsewhere in between gets another interleaving
(``workers_per_gpu=0`` draws on the consuming thread, nothing ahead).

Lookahead is bounded.  A batch counts as consumed when the consumer comes back for the next one.  Batch ``k`` is begun only
once batch ``k - prefetch`` is consumed, and the decode of the sample at place ``p`` of the order is started only once
``p < consumed samples + prefetch * batch_size + workers`` -- beside the batch in the consumer's hands at most ``prefetch``
finished batches and ``workers`` decoded images are held.

Failure.  An exception on a background thread is kept with the batch that needed the failed sample and re-raised, with its
type, by the ``next()`` that asks for that batch; earlier batches are delivered.  Every wait of the consumer is on one condition
variable that the producers notify when they publish, fail or end, so a dead producer wakes it.  Leaving the loop,
``close()`` and garbage collection stop and join every thread of the epoch.

Only the consuming thread calls into HIP.  Background threads write host memory only, page-locked ring slots included; the
consumer allocates the slots, issues every upload and launch from inside ``__next__`` on its current stream, and a slot is
written again only after the event recorded behind its upload has completed.  That keeps the feed legal next to a stream
capture on the consuming thread and the process at one GPU context.  No side stream is used: on one in-order stream the
upload of a batch is issued when the batch is handed out (issuing it one batch earlier would change nothing there).

``device_decode=True`` (with ``device_preprocess=True``): the pool only reads the files and parses their headers
(``dataset.load_image_file``), the draws and plans use the header's shape, ``_stage`` packs the files' bytes into the ring slot
behind the ground truth, and the consumer decodes the batch in one ``kgdet_jpeg_decode`` call (``jpeg.DeviceDecodeRoute``)
before ``collate_device``.  The batches are bit for bit those of ``device_decode=False``.  A batch is handed out only once the
decoder's status is known: an image it refused is decoded by PIL on the spot, with a warning.  This route DOES use a side
stream, for the block's upload, the decode and the status read-back, so that the read-back never waits for the training
step queued on the consumer's stream; that stream then waits for the decode's event.  When the next batch is already
staged as a batch is handed out, its upload and decode are issued right then (one batch ahead, nothing waited for), so they run
under the training step and the next ``__next__`` should find the status there (measured, README: it still waits 4 to 5 ms
per batch, against 1.3 to 2.9 ms of the threaded PIL route -- the decode call is slower under the step).  A file the decoder does not take
(progressive, 4:2:2, ...) is decoded by PIL in the pool, as on the other routes.  ``device_decode='camera'`` is the same route
with ``jpeg.parse_header(camera=True)`` and ``kgdet_jpeg_decode_camera``: 4:2:2 files and files with restart intervals are
decoded on the device too, without a warning; the rest of that list still goes to PIL.  The resample of an image without annotations
reads that image's file on the drawing thread (the other routes decode it there) and it is decoded on the GPU with its batch.
"""
import functools
import threading
import weakref
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import datasets as ds

MAX_WORKERS = 16
_RAW_KEYS = ('raw', 'scale', 'flip', 'keep_ratio', 'img_meta', 'aug_plan')


def draw_train_raw(dataset, idx, img=None, load=None):
    """``dataset[idx]``'s loop around ``prepare_train_raw``: the sample's draws, and for an image without annotations
    (``skip_img_without_anno``) the resample of ``__getitem__`` -- ``np.random.choice`` within the aspect-ratio group, then
    that image decoded here.  ``img``: the decoded image of ``idx`` when somebody decoded it ahead.  ``load``: what reads an
    image nobody read ahead (``dataset.load_image_file`` on the ``device_decode`` route, so that a resampled image travels as
    its file too; default: ``prepare_train_raw``'s own ``load_image``)."""
    while True:
        if img is None and load is not None:
            img = load(idx)
        raw = dataset.prepare_train_raw(idx, img=img)
        if raw is not None:
            return raw
        idx = int(np.random.choice(np.where(dataset.flag == dataset.flag[idx])[0]))
        img = None


def _align(n, a):
    return (n + a - 1) // a * a


def gt_layout(samples):
    """Where every ground-truth tensor of a batch lies in ONE byte block: ``(entries, nbytes)`` with ``entries`` a list of
    ``(key, shape, dtype, offset)`` in hand-out order per key; the tensors with the widest elements (the int64 labels) come
    first, so every offset is a multiple of its element size."""
    keys = [k for k in samples[0] if k not in _RAW_KEYS and k != 'img']
    items = [(k, s[k]) for k in keys for s in samples]
    order = sorted(range(len(items)), key=lambda j: -items[j][1].element_size())
    offsets, at = [0] * len(items), 0
    for j in order:
        t = items[j][1]
        at = _align(at, t.element_size())
        offsets[j] = at
        at += t.numel() * t.element_size()
    return [(k, tuple(t.shape), t.dtype, o) for (k, t), o in zip(items, offsets)], at


def _view(block, shape, dtype, offset):
    n = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    return block[offset:offset + n].view(dtype).view(shape)


class _Staged(object):
    """one finished batch on the host: ``block`` (uint8: the packed ground truth and, on the host route, the collated
    image behind it), its layout, and what stays on the host"""

    def __init__(self, block, entries, nbytes, img_at, img_shape, metas, samples, files_at=None, places=None):
        self.block, self.entries, self.nbytes = block, entries, nbytes
        self.img_at, self.img_shape, self.metas, self.samples = img_at, img_shape, metas, samples
        self.files_at, self.places = files_at, places      # device_decode: the files' bytes in the block (jpeg.pack_files)


def _encoded(samples):
    """the files of a batch the device decodes: (bytes, frame) of every ``EncodedImage`` that has a frame, in order"""
    raws = [s['raw'] for s in samples]
    keep = [r for r in raws if isinstance(r, ds.EncodedImage) and r.frame is not None]
    return [r.data for r in keep], [r.frame for r in keep]


def _stage(samples, raw_route, slot_block, decode=False):
    """pack a batch for upload (host memory only): into ``slot_block`` when it is large enough, else into a pageable block of
    the same layout, which the consumer moves into a slot it has grown.  ``decode``: the files' bytes follow the ground truth"""
    entries, gt_bytes = gt_layout(samples)
    files_at = places = None
    if raw_route and decode:
        from . import jpeg
        files, frames = _encoded(samples)
        img_at, img_shape, files_at = None, None, _align(gt_bytes, 256)
        total = files_at + jpeg.pack_files(files, frames)[0]
    elif raw_route:
        img_at, img_shape, total = None, None, gt_bytes
    else:
        H = max(s['img'].shape[1] for s in samples)
        W = max(s['img'].shape[2] for s in samples)
        img_at, img_shape = _align(gt_bytes, 256), (len(samples), 3, H, W)
        total = img_at + 4 * len(samples) * 3 * H * W
    block = slot_block if slot_block is not None and slot_block.numel() >= total else torch.empty(max(total, 1), dtype=torch.uint8)
    per_key = {}
    for key, shape, dtype, off in entries:
        src = samples[per_key.setdefault(key, 0)][key]
        per_key[key] += 1
        _view(block, shape, dtype, off).copy_(src)
    if not raw_route:
        img = _view(block, img_shape, torch.float32, img_at)
        img.zero_()
        for i, s in enumerate(samples):
            img[i, :, :s['img'].shape[1], :s['img'].shape[2]] = s['img']
    if files_at is not None:
        _, places = jpeg.pack_files(files, frames, block.numpy()[files_at:total])
    return _Staged(block, entries, total, img_at, img_shape, [s['img_meta'] for s in samples], samples if raw_route else None,
                   files_at, places)


class _Epoch(object):
    """the shared state of one epoch in flight; the threads hold this object and never the iterator, so dropping the iterator
    ends them"""

    def __init__(self, loader, order):
        self.dataset, self.B, self.prefetch = loader.dataset, loader.batch_size, max(loader.prefetch, 1)
        self.workers, self.raw_route, self.staged = loader.workers, loader.device_preprocess, loader.device is not None
        self.decode = loader.device_decode
        self.load = loader._load_file() if self.decode else loader.dataset.load_image
        self.slots = loader._slots
        self.order = order
        self.n_batches = -(-len(order) // self.B)
        self.cv = threading.Condition()
        self.done = {}                 # batch number -> ('ok', value) | ('error', exception)
        self.consumed = 0              # batches the consumer has come back from
        self.stop = False
        self.producer_ended = False
        self.decodes = {}              # place in the order -> future of load_image
        self.next_decode = 0
        self.submitted = 0             # batches handed to the pool for assembly
        self.pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix='kgdet-loader')
        self.thread = threading.Thread(target=self._produce, name='kgdet-loader-draws', daemon=True)
        self.thread.start()

    # ---- background side -------------------------------------------------------------------------
    def _publish(self, k, kind, value):
        with self.cv:
            self.done.setdefault(k, (kind, value))
            self.cv.notify_all()

    def _submit_decodes(self):
        """start the decodes the window allows (called with ``cv`` held)"""
        limit = min(len(self.order), (self.consumed + self.prefetch) * self.B + self.workers)
        while self.next_decode < limit and not self.stop:
            p = self.next_decode
            self.decodes[p] = self.pool.submit(self.load, self.order[p])
            self.next_decode += 1

    def _produce(self):
        k = 0
        try:
            for k in range(self.n_batches):
                with self.cv:
                    while not self.stop and k >= self.consumed + self.prefetch:
                        self.cv.wait()
                    if self.stop:
                        return
                    self._submit_decodes()
                places = range(k * self.B, min((k + 1) * self.B, len(self.order)))
                futures = []
                for p in places:
                    with self.cv:
                        if self.stop:
                            return
                        fut = self.decodes.pop(p)
                    raw = draw_train_raw(self.dataset, self.order[p], fut.result(), self.load if self.decode else None)
                    futures.append(raw if self.raw_route else self.pool.submit(ds.finish_train_sample, self.dataset, raw))
                self.pool.submit(self._assemble, k, futures)
                with self.cv:
                    self.submitted = k + 1
        except BaseException as e:     # (the batch that needed the sample carries it; nothing is drawn after a failure)
            self._publish(k, 'error', e)
        finally:
            with self.cv:
                self.producer_ended = True
                self.cv.notify_all()

    def _assemble(self, k, futures):
        try:
            samples = futures if self.raw_route else [f.result() for f in futures]
            if self.staged:
                slot = self.slots[k % len(self.slots)]
                value = _stage(samples, self.raw_route, slot.block, self.decode)
            else:
                value = samples if self.raw_route else ds.collate(samples)
            self._publish(k, 'ok', value)
        except BaseException as e:
            self._publish(k, 'error', e)

    # ---- consumer side ---------------------------------------------------------------------------
    def take(self, k):
        """batch ``k`` (blocking), or raise what its samples raised; ``StopIteration`` past the end or after ``close``"""
        with self.cv:
            lost = ('error', RuntimeError('the loader\'s producer ended without batch %d' % k))
            while k not in self.done and not self.stop and k < self.n_batches:
                if self.producer_ended and k >= self.submitted:      # (a guard: every way out of the producer publishes)
                    self.done[k] = lost
                    break
                self.cv.wait(1.0)
            kind, value = self.done.pop(k, ('end', None))
        if kind == 'ok':
            return value
        self.close()
        if kind == 'error':
            raise value
        raise StopIteration

    def take_if_ready(self, k):
        """batch ``k`` if it is finished and sound, without waiting (else None: ``take`` will wait for it or raise its error)"""
        with self.cv:
            if k in self.done and self.done[k][0] == 'ok' and not self.stop:
                return self.done.pop(k)[1]
        return None

    def came_back(self):
        with self.cv:
            self.consumed += 1
            self._submit_decodes()
            self.cv.notify_all()

    def close(self):
        with self.cv:
            if self.stop:
                return
            self.stop = True
            self.cv.notify_all()
        self.pool.shutdown(wait=False, cancel_futures=True)
        if threading.current_thread() is not self.thread:
            self.thread.join()
        self.pool.shutdown(wait=True)
        with self.cv:
            self.done.clear()
            self.decodes.clear()


class _Slot(object):
    """one page-locked ring slot: allocated and grown by the consumer, written by the pool, free again once ``event`` -- recorded
    behind the upload out of it -- has completed"""

    def __init__(self):
        self.block, self.event = None, None


class _LoaderIter(object):
    def __init__(self, loader, order):
        self.loader, self.k, self.begun = loader, 0, None
        self.epoch = _Epoch(loader, order)
        loader._active = weakref.ref(self.epoch)

    def __iter__(self):
        return self

    def __next__(self):
        loader, ep, k = self.loader, self.epoch, self.k
        if k > 0:
            # the consumer is back: batch k - 1 counts as consumed, which lets the producers begin batch k - 1 + prefetch.  The
            # slot that one is written into is the one batch k - 3 went up from (prefetch + 2 slots): its upload has to be over
            old = loader._slots[(k - 3) % len(loader._slots)] if ep.staged and k >= 3 else None
            if old is not None and old.event is not None:
                old.event.synchronize()
            ep.came_back()
        if self.begun is not None:             # device_decode: this batch's decode was issued while the last one was in use
            begun, self.begun = self.begun, None
        else:
            begun = ep.take(k)
            if ep.staged:
                begun = loader._begin_upload(begun, loader._slots[k % len(loader._slots)])
        try:
            value = loader._end_upload(begun) if ep.staged else begun
            if ep.decode:
                nxt = ep.take_if_ready(k + 1)
                if nxt is not None:            # (its slot last sent batch k - 3 or an earlier one: synchronised above)
                    self.begun = loader._begin_upload(nxt, loader._slots[(k + 1) % len(loader._slots)])
        except BaseException:                  # (PIL's error for a file the device refused: the epoch ends as in ``take``)
            ep.close()
            raise
        self.k = k + 1
        return value

    def close(self):
        self.epoch.close()

    def __del__(self):
        try:
            self.epoch.close()
        except Exception:
            pass


class DataLoader(object):
    """what ``build_dataloader`` returns: iterate it once per epoch (``Runner.run(loader, ..., set_epoch=loader.set_epoch)``);
    the module docstring states what it yields and guarantees"""

    def __init__(self, dataset, batch_size, workers, sampler=None, device=None, device_preprocess=False, prefetch=2,
                 device_decode=False):
        if workers < 0 or prefetch < 0 or batch_size < 1:
            raise ValueError('workers and prefetch are >= 0 and the batch size >= 1, got %r, %r, %r'
                             % (workers, prefetch, batch_size))
        self.dataset, self.batch_size, self.sampler = dataset, int(batch_size), sampler
        self.workers = min(int(workers), MAX_WORKERS)      # a thread count, never sized from the machine
        self.prefetch, self.device_preprocess = int(prefetch), bool(device_preprocess)
        from .jpeg import decode_switch
        self.device_decode, self.decode_camera = decode_switch(device_decode)       # (True or 'camera', which also takes 4:2:2 and DRI files)
        if self.device_decode and not (self.device_preprocess and device is not None):
            raise ValueError('device_decode=True needs device_preprocess=True and a device: the decoded images stay on the GPU')
        if self.device_decode and self.batch_size > 32:
            raise ValueError('device_decode=True decodes a batch in one call of at most 32 images, got %d' % self.batch_size)
        self.device, self._route = None, None
        self._active = lambda: None
        self._slots, self._transform = [], None
        if device is not None:
            device = torch.device(device)
            if device.type != 'cuda':
                raise ValueError('device is None (host batches) or a CUDA device, got %s' % device)
            if not torch.cuda.is_available():
                raise RuntimeError('device=%s asked for, but no GPU is available' % device)
            self.device = torch.device('cuda', torch.cuda.current_device() if device.index is None else device.index)
            # batch k is written while k - 1 .. k - prefetch wait and k - prefetch - 1 may still be going up
            self._slots = [_Slot() for _ in range(max(self.prefetch, 1) + 2)]
            if self.device_preprocess:
                self._transform = dataset.device_transform(self.device)
            if self.device_decode:
                from .jpeg import DeviceDecodeRoute
                self._route = DeviceDecodeRoute(self.device, self.decode_camera)

    def _load_file(self):
        """the dataset's ``load_image_file`` with the loader's ``camera`` switch (looked up on the ``device_decode`` routes only)"""
        load = self.dataset.load_image_file
        return functools.partial(load, camera=True) if self.decode_camera else load

    def __len__(self):
        n = len(self.dataset) if self.sampler is None else len(self.sampler)
        return -(-n // self.batch_size)

    def set_epoch(self, epoch):
        if hasattr(self.sampler, 'set_epoch'):
            self.sampler.set_epoch(epoch)

    def close(self):
        """end the epoch in flight, if any: every thread is stopped and joined"""
        ep = self._active()
        if ep is not None:
            ep.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _order(self):
        return list(range(len(self.dataset))) if self.sampler is None else [int(i) for i in self.sampler]

    def __iter__(self):
        self.close()
        order = self._order()
        if self.workers == 0:
            return self._serial(order)
        for slot in self._slots:           # (an epoch that was left early: its uploads are over before a slot is written again)
            if slot.event is not None:
                slot.event.synchronize()
                slot.event = None
        self._presize()
        return _LoaderIter(self, order)

    # ---- the serial loop: the definition ---------------------------------------------------------
    def _serial(self, order):
        B, data = self.batch_size, self.dataset
        for lo in range(0, len(order), B):
            if self.device_preprocess:
                samples = [draw_train_raw(data, i, None, self._load_file() if self.device_decode else None) for i in order[lo:lo + B]]
                if self.device is None:
                    yield samples
                    continue
            else:
                samples = [data[i] for i in order[lo:lo + B]]
                if self.device is None:
                    yield ds.collate(samples)
                    continue
            slot = _Slot()                 # nothing runs ahead: a buffer per batch, kept alive by the caching host allocator
            yield self._upload(_stage(samples, self.device_preprocess, None, self.device_decode), slot)

    # ---- consumer-side GPU work ------------------------------------------------------------------
    def _presize(self):
        """allocate the ring slots (this thread is the consumer) at the size the dataset's scales bound, so the pool writes
        page-locked memory from the first batch on; a batch that is larger still goes through ``_upload``'s growth"""
        if not self._slots or self._slots[0].block is not None:
            return
        need = 1 << 20
        scales = getattr(self.dataset, 'img_scales', None)
        if not self.device_preprocess and scales:
            div = getattr(self.dataset, 'size_divisor', None) or 1
            long_edge, short_edge = max(max(s) for s in scales), max(min(s) for s in scales)
            need += 12 * self.batch_size * _align(long_edge, div) * _align(short_edge, div)
        for slot in self._slots:
            slot.block = torch.empty(need, dtype=torch.uint8, pin_memory=True)

    def _upload(self, staged, slot):
        """one non-blocking copy of the staged block out of page-locked memory on the current stream of ``device``, the event
        behind it recorded in ``slot``; the batch dict with device views (``img`` through ``collate_device`` on the raw route)"""
        return self._end_upload(self._begin_upload(staged, slot))

    def _begin_upload(self, staged, slot):
        """the first half of ``_upload``: everything that waits for nothing.  On the ``device_decode`` route that is the block's
        upload, the decode and the status read-back, issued on the route's stream; on the others it is all of ``_upload``"""
        with torch.cuda.device(self.device):
            if staged.block is not slot.block:        # the slot was too small (or absent): grow it here, on the consumer
                if slot.event is not None:
                    slot.event.synchronize()
                if slot.block is None or slot.block.numel() < staged.nbytes:
                    slot.block = torch.empty(_align(staged.nbytes + staged.nbytes // 4, 4096), dtype=torch.uint8, pin_memory=True)
                slot.block[:staged.nbytes].copy_(staged.block[:staged.nbytes])
            if staged.files_at is not None:           # device_decode: upload, decode and status on the route's own stream
                pending = self._route.start_block(slot.block[:staged.nbytes], staged.files_at, staged.places,
                                                  [s['raw'] for s in staged.samples])
                slot.event = pending.uploaded
                return staged, pending
            else:
                dev = slot.block[:staged.nbytes].to(self.device, non_blocking=True)
                slot.event = torch.cuda.Event()
                slot.event.record()
                if staged.samples is not None:
                    out = dict(img=ds.collate_device(staged.samples, self._transform)['img'], img_meta=staged.metas)
                else:
                    out = dict(img=_view(dev, staged.img_shape, torch.float32, staged.img_at), img_meta=staged.metas)
            for key, shape, dtype, off in staged.entries:
                out.setdefault(key, []).append(_view(dev, shape, dtype, off))
        return out

    def _end_upload(self, begun):
        """the second half: the batch dict.  ``device_decode``: waits for the decode's event alone (the status), then the
        preprocess launch on the current stream"""
        if not isinstance(begun, tuple):
            return begun
        staged, pending = begun
        with torch.cuda.device(self.device):
            dev, raws = self._route.finish_block(pending)
            samples = [dict(s, raw=r) for s, r in zip(staged.samples, raws)]
            out = dict(img=ds.collate_device(samples, self._transform)['img'], img_meta=staged.metas)
            for key, shape, dtype, off in staged.entries:
                out.setdefault(key, []).append(_view(dev, shape, dtype, off))
        return out


def build_dataloader(dataset, imgs_per_gpu, workers_per_gpu, num_gpus=1, dist=False, shuffle=True, *, device=None,
                     device_preprocess=False, prefetch=2, sampler=None, device_decode=False):
    """``mmdet.datasets.build_dataloader`` for one process.  ``shuffle=True``: ``GroupSampler`` (``dist=False``; batches of
    ``num_gpus * imgs_per_gpu``) or ``DistributedGroupSampler`` (``dist=True``); ``shuffle=False``: dataset order (this rank's
    ``runner.test_shard`` with ``dist=True``); ``sampler``: any iterable of indices with a ``len`` instead.  ``workers_per_gpu``:
    the decode pool's THREADS (times ``num_gpus`` without ``dist``, as the reference counts them), capped at 16; 0: the serial
    loop on the consuming thread.  ``prefetch``: finished batches held ahead.  ``device=None`` yields ``datasets.collate``'s host
    batch -- with ``device_preprocess=True`` the list of ``prepare_train_raw`` samples ``datasets.collate_device`` takes --;
    ``device='cuda[:n]'`` yields the batch dict on the GPU (``model(**data)``, ``GraphedTrainStep.load``): the ground truth as
    views of ONE uploaded block, ``img`` from ``collate_device`` (one launch) or, on the host route, from the same page-locked
    block; ``img_meta`` stays a host list.  ``device_decode=True`` or ``'camera'`` (the latter also decodes 4:2:2 files and files
    with restart intervals on the device: ``jpeg.parse_header(camera=True)``; both need ``device_preprocess=True`` and a ``device``, else
    ``ValueError``): the JPEG files are decoded on the GPU too, the same batches bit for bit.  The determinism, lookahead,
    failure and threading contracts: the module docstring."""
    if workers_per_gpu < 0 or prefetch < 0:
        raise ValueError('workers_per_gpu and prefetch are >= 0, got %r and %r' % (workers_per_gpu, prefetch))
    if dist:
        batch_size, workers = imgs_per_gpu, workers_per_gpu
    else:
        batch_size, workers = num_gpus * imgs_per_gpu, num_gpus * workers_per_gpu
    if sampler is None:
        if shuffle:
            sampler = (ds.DistributedGroupSampler(dataset, imgs_per_gpu) if dist else ds.GroupSampler(dataset, imgs_per_gpu))
        elif dist:
            import torch.distributed as td
            from .runner import test_shard
            on = td.is_available() and td.is_initialized()
            sampler = test_shard(len(dataset), td.get_world_size() if on else 1, td.get_rank() if on else 0)
    return DataLoader(dataset, batch_size, workers, sampler=sampler, device=device, device_preprocess=device_preprocess,
                      prefetch=prefetch, device_decode=device_decode)
