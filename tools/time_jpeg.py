"""Time the JPEG encoder of the drawn pictures: ``kgdet_jpeg_encode`` / ``kgdet_jpeg_write`` alone, and ``single_gpu_test`` without
``show_dir``, with ``show_encoder='host'`` and with ``show_encoder='device'``.

    python tools/time_jpeg.py [--batch 8] [--sizes 624x468,800x1088] [--rows 100] [--windows 9] [--iters 10]
    python tools/time_jpeg.py --loop [--images 256] [--workers 4] [--show-score-thr 0.05]

Kernel legs: ``--batch`` pictures of one size (H x W: blocks of 32 x 32 pixels of one colour under noise of sigma 6, as the demo
set is rendered, with ``--rows`` detections drawn on each by ``visualize.DeviceDrawer``) lie in the drawer's destination buffer
and are encoded where they lie: ``--windows`` windows of ``--iters`` calls between two events.  Per leg: the microseconds per
image of ``kgdet_jpeg_encode`` after each of its five kernels (KGDET_JPEG_STOP_AFTER = 1 .. 5: the differences are the kernels'
own times) and of ``kgdet_jpeg_write`` (median of the windows, min and max), the bytes read + written per image (pixels,
coefficients written and read twice, the stream written and read, the file) and their rate against the 6.29 TB/s of a float4
copy, once the check that the first file equals ``jpeg_restatement``, and PIL's encode of the same arrays (quality 90) on 1 and
on 4 threads, in microseconds per image.

``--loop``: the loop of tools/time_draw.py ``--loop`` (the image set of tools/time_loader.py, ``single_gpu_test`` under bf16
autocast with ``imgs_per_gpu=8``, ``device_preprocess`` and ``device_results`` on at ``--workers``) without ``show_dir``, with
``show_encoder='host'`` and with ``show_encoder='device'``, in one process, alternated twice after a warm-up: wall seconds, the
bytes handed to the writer per image (what came down from the GPU) and the thread-seconds inside the writer's threads.  Prints
one JSON line."""
import argparse
import importlib.util
import io
import json
import os
import shutil
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TB_S = 6.29


def _tool(name):
    spec = importlib.util.spec_from_file_location('kgdet_tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def rendered(rng, H, W):
    coarse = rng.integers(40, 216, (H // 32 + 2, W // 32 + 2, 3)).astype(np.float32)
    img = np.kron(coarse, np.ones((32, 32, 1), np.float32))[:H, :W]
    img += rng.normal(0, 6.0, img.shape).astype(np.float32)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def event_us(fn, windows, iters):
    import torch
    times = []
    for _ in range(windows):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end) * 1e3 / iters)
    return times


def kernel_legs(args):
    import ctypes
    from concurrent.futures import ThreadPoolExecutor
    import torch
    from PIL import Image
    from kgdet_amd import _lib, jpeg
    from kgdet_amd import visualize as vz
    from kgdet_amd.evaluation import landmark_meta
    time_draw = _tool('time_draw')
    meta = landmark_meta()
    names, ranges = meta['classes'], meta['landmark_ranges']
    lib, p, i32, i64, sz = _lib.lib(), _lib.ptr, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    legs = []
    for size in args.sizes.split(','):
        H, W = (int(v) for v in size.split('x'))
        rng = np.random.default_rng(H * 10000 + W)
        n = args.batch
        images = [rendered(rng, H, W) for _ in range(n)]
        rows = torch.from_numpy(time_draw.make_rows(H + W, n, args.rows, H, W, len(names))).cuda()
        stride = (3 * H * W + 255) // 256 * 256
        offsets, shapes = [k * stride for k in range(n)], [(H, W)] * n
        src = torch.zeros(stride * n, dtype=torch.uint8, device='cuda')
        for k, img in enumerate(images):
            src[offsets[k]:offsets[k] + img.size].copy_(torch.from_numpy(img.reshape(-1)))
        drawn = torch.zeros_like(src)
        vz.DeviceDrawer(names, landmark_ranges=ranges).launch(src, drawn, offsets, shapes, rows, list(range(n)))
        pictures = [drawn[o:o + 3 * H * W].view(H, W, 3) for o in offsets]
        arrays = [t.cpu().numpy() for t in pictures]
        files = jpeg.DeviceJpegEncoder(90)(pictures)
        equal = files[0] == jpeg.jpeg_restatement(arrays[0])
        table = (i64 * (4 * n))(*[v for k in range(n) for v in (offsets[k], 0, H, W)])
        ws = torch.empty(lib.kgdet_jpeg_workspace_bytes(table, i32(n)), dtype=torch.uint8, device='cuda')
        lengths = torch.empty(n, dtype=torch.int64, device='cuda')
        stream = _lib.current_stream()

        def encode():
            _lib.check(lib.kgdet_jpeg_encode(p(drawn), i64(drawn.numel()), table, i32(n), i32(90), p(ws), sz(ws.numel()), p(lengths),
                                             stream), 'kgdet_jpeg_encode')
        stages = {}
        for stop, kernel in enumerate(('transform', 'measure', 'scan_bits', 'pack', 'scan_ff'), 1):
            os.environ['KGDET_JPEG_STOP_AFTER'] = str(stop)
            encode()
            t = [v / n for v in event_us(encode, args.windows, args.iters)]
            stages[kernel] = dict(cum_us=round(float(np.median(t)), 2), us_min=round(min(t), 2), us_max=round(max(t), 2))
        del os.environ['KGDET_JPEG_STOP_AFTER']
        sizes = [int(v) for v in lengths.cpu().tolist()]
        place, total = [], 0
        for s in sizes:
            place.append(total)
            total += (s + 15) // 16 * 16
        table = (i64 * (4 * n))(*[v for k in range(n) for v in (offsets[k], place[k], H, W)])
        out = torch.empty(total, dtype=torch.uint8, device='cuda')
        status = torch.empty(n, dtype=torch.int32, device='cuda')
        capacity = (i64 * n)(*sizes)

        def write():
            _lib.check(lib.kgdet_jpeg_write(table, i32(n), i32(90), p(ws), sz(ws.numel()), capacity, p(out), i64(total), p(status),
                                            stream), 'kgdet_jpeg_write')
        write()
        t = [v / n for v in event_us(write, args.windows, args.iters)]
        stages['finish'] = dict(us=round(float(np.median(t)), 2), us_min=round(min(t), 2), us_max=round(max(t), 2))
        assert out[place[0]:place[0] + sizes[0]].cpu().numpy().tobytes() == files[0] and not status.any()

        def pil(a):
            buf = io.BytesIO()
            Image.fromarray(a).save(buf, format='JPEG', quality=90)
            return buf.tell()
        pil_us = {}
        for threads in (1, 4):
            with ThreadPoolExecutor(threads) as pool:
                list(pool.map(pil, arrays))
                t = []
                for _ in range(args.windows):
                    t0 = time.perf_counter()
                    pil_bytes = sum(pool.map(pil, arrays))
                    t.append((time.perf_counter() - t0) * 1e6 / n)
            pil_us[threads] = dict(us=round(float(np.median(t)), 1), us_min=round(min(t), 1), us_max=round(max(t), 1))
        mcus = ((H + 15) // 16) * ((W + 15) // 16)
        mean_file = sum(sizes) / n
        moved = 3 * H * W + 3 * 768 * mcus + 3 * mean_file
        us = stages['scan_ff']['cum_us'] + stages['finish']['us']
        legs.append(dict(size='%dx%d' % (H, W), batch=n, rows=args.rows, equals_restatement=bool(equal), stages=stages,
                         us_per_image=round(us, 2), bytes_per_image=int(moved), file_bytes=int(mean_file), pil_file_bytes=pil_bytes // n,
                         tb_s=round(moved / us / 1e6, 4), of_copy=round(moved / us / 1e6 / COPY_TB_S, 4), pil_us_per_image=pil_us,
                         cpus_usable=len(os.sched_getaffinity(0))))
        print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    return legs


def loop_legs(args):
    import torch
    from kgdet_amd import configs
    from kgdet_amd import datasets as ds
    from kgdet_amd import runner as rn
    from kgdet_amd import visualize as vz
    from kgdet_amd.registry import build_detector
    from tests.golden import demo_cases
    time_loader = _tool('time_loader')
    torch.backends.cudnn.benchmark = False
    tmp = tempfile.mkdtemp(prefix='kgdet_jpeg_')
    spent = dict(writer_thread_s=0.0, bytes=0)
    lock = threading.Lock()
    host_write, bytes_write = vz.PictureWriter._write, vz.PictureWriter._write_bytes

    def timed(fn):
        def inner(self, data, name):
            t0 = time.perf_counter()
            try:
                return fn(self, data, name)
            finally:
                with lock:
                    spent['writer_thread_s'] += time.perf_counter() - t0
                    spent['bytes'] += data.nbytes if hasattr(data, 'nbytes') else len(data)
        return inner
    try:
        ann_file, prefix = time_loader.render_image_dir(tmp, args.images)
        data = ds.DeepFashion2Dataset(ann_file=ann_file, img_prefix=prefix, img_scale=demo_cases.IMG_SCALE,
                                      img_norm_cfg=demo_cases.IMG_NORM, size_divisor=32, with_mask=False, with_crowd=False,
                                      with_keypoint=True, flip_ratio=0, with_label=False, test_mode=True)
        cfg = configs.kgdet_r50_fpn()
        torch.manual_seed(0)
        model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
        demo_cases.spread_head(model.bbox_head)
        model = model.cuda().eval()

        def run(show_dir, encoder='host'):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.autocast('cuda', dtype=torch.bfloat16):
                rn.single_gpu_test(model, data, imgs_per_gpu=8, device_preprocess=True, device_results=True, workers=args.workers,
                                   show_dir=show_dir, show_score_thr=args.show_score_thr, show_encoder=encoder).release()
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        run(None)                                        # every shape of the set once
        run(os.path.join(tmp, 'warm'), 'device')
        vz.PictureWriter._write, vz.PictureWriter._write_bytes = timed(host_write), timed(bytes_write)
        out = dict(images=args.images, workers=args.workers, show_score_thr=args.show_score_thr, plain_s=[], host_s=[], device_s=[],
                   host_writer_thread_s=[], device_writer_thread_s=[], cpus_usable=len(os.sched_getaffinity(0)))
        for k in range(2):
            out['plain_s'].append(round(run(None), 3))
            for encoder in ('host', 'device'):
                spent.update(writer_thread_s=0.0, bytes=0)
                shown = os.path.join(tmp, '%s%d' % (encoder, k))
                out[encoder + '_s'].append(round(run(shown, encoder), 3))
                out[encoder + '_writer_thread_s'].append(round(spent['writer_thread_s'], 3))
                out[encoder + '_bytes_down_per_image'] = spent['bytes'] // args.images
                out[encoder + '_pictures'] = len(os.listdir(shown))
                out[encoder + '_file_bytes_per_image'] = sum(os.path.getsize(os.path.join(shown, f)) for f in os.listdir(shown)) // args.images
            print('round %d: %s' % (k, json.dumps(out)), file=sys.stderr, flush=True)
        return out
    finally:
        vz.PictureWriter._write, vz.PictureWriter._write_bytes = host_write, bytes_write
        shutil.rmtree(tmp, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--sizes', default='624x468,800x1088', help='H x W, comma separated')
    ap.add_argument('--rows', type=int, default=100)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--loop', action='store_true')
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--workers', type=int, default=4)
    ap.add_argument('--show-score-thr', type=float, default=0.05)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_jpeg.py needs a GPU')
    out = dict(loop=loop_legs(args)) if args.loop else dict(kernel=kernel_legs(args))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
