"""Time the drawing of detections: ``kgdet_draw_detections`` alone, and ``single_gpu_test`` with and without ``show_dir``.

    python tools/time_draw.py [--batch 8] [--sizes 624x468,800x1088] [--rows 100] [--windows 9] [--iters 20]
    python tools/time_draw.py --loop [--images 256] [--workers 4]

Kernel legs: ``--batch`` images of one size (H x W, seeded noise) with ``--rows`` rows each, all above the threshold: boxes
about the image, K = 294 landmarks scattered about their box, all visible, DeepFashion2's ranges (a category draws its own 25
to 39), with the contour off and on.  The images lie in one flat device buffer and ``visualize.DeviceDrawer.launch`` draws
them into another, one launch per call: ``--windows`` windows of ``--iters`` calls between two events.
Per leg: the microseconds per image (median of the windows, min and max), the bytes moved (source read + destination
written) and their rate against the 6.29 TB/s of a float4 copy, and once the check that the picture equals
``draw_restatement`` on the first image.

``--loop``: the image set of tools/time_loader.py (``--images`` rendered JPEGs), ``single_gpu_test`` under bf16 autocast with
``imgs_per_gpu=8``, ``device_preprocess`` and ``device_results`` on at ``--workers``: wall seconds without ``show_dir`` and
with it (JPEG, into a temporary directory), twice each after a warm-up, and of the run with pictures the seconds inside
``DeviceDrawer`` calls (draw + download, on the loop's thread) and the thread-seconds inside the encoder (``save_image``, summed
over the writer threads).  Prints one JSON line."""
import argparse
import importlib.util
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


def make_rows(seed, n, M, H, W, L, K=294):
    rng = np.random.default_rng(seed)
    block = np.zeros((n, M, 7 + 3 * K), dtype=np.float32)
    cx, cy = rng.uniform(0.1 * W, 0.9 * W, (n, M)), rng.uniform(0.1 * H, 0.9 * H, (n, M))
    bw, bh = rng.uniform(0.1 * W, 0.6 * W, (n, M)), rng.uniform(0.1 * H, 0.6 * H, (n, M))
    block[..., 0], block[..., 1], block[..., 2], block[..., 3] = cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2
    block[..., 4] = rng.uniform(0.31, 1.0, (n, M))
    block[..., 5] = rng.integers(0, L, (n, M))
    block[..., 6] = M
    pts = block[..., 7:].reshape(n, M, K, 3)
    pts[..., 0] = cx[..., None] + rng.uniform(-0.5, 0.5, (n, M, K)) * bw[..., None]
    pts[..., 1] = cy[..., None] + rng.uniform(-0.5, 0.5, (n, M, K)) * bh[..., None]
    pts[..., 2] = 1.0
    return block


def kernel_legs(args):
    import torch
    from kgdet_amd import visualize as vz
    from kgdet_amd.evaluation import landmark_meta
    meta = landmark_meta()
    names, ranges = meta['classes'], meta['landmark_ranges']
    legs = []
    for size in args.sizes.split(','):
        H, W = (int(v) for v in size.split('x'))
        rng = np.random.default_rng(H * 10000 + W)
        images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(args.batch)]
        block = make_rows(H + W, args.batch, args.rows, H, W, len(names))
        rows = torch.from_numpy(block).cuda()
        for contour in (False, True):
            drawer = vz.DeviceDrawer(names, landmark_ranges=ranges, contour=contour)
            stride = (3 * H * W + 255) // 256 * 256
            offsets, shapes, blocks = [k * stride for k in range(args.batch)], [(H, W)] * args.batch, list(range(args.batch))
            src = torch.zeros(stride * args.batch, dtype=torch.uint8, device='cuda')
            for k, img in enumerate(images):
                src[offsets[k]:offsets[k] + img.size].copy_(torch.from_numpy(img.reshape(-1)))
            dst = torch.zeros_like(src)
            for _ in range(3):
                drawer.launch(src, dst, offsets, shapes, rows, blocks)
            first = dst[:3 * H * W].view(H, W, 3).cpu().numpy()
            equal = bool(np.array_equal(first, vz.draw_restatement(images[0], block[0], args.rows, names, landmark_ranges=ranges,
                                                                  contour=contour)))
            times = []
            for _ in range(args.windows):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(args.iters):
                    drawer.launch(src, dst, offsets, shapes, rows, blocks)
                end.record()
                end.synchronize()
                times.append(start.elapsed_time(end) * 1e3 / args.iters / args.batch)
            moved = 2 * 3 * H * W
            med = float(np.median(times))
            legs.append(dict(size='%dx%d' % (H, W), batch=args.batch, rows=args.rows, contour=contour, equals_restatement=equal,
                             us_per_image=round(med, 2), us_min=round(min(times), 2), us_max=round(max(times), 2),
                             bytes_per_image=moved, tb_s=round(moved / med / 1e6, 4),
                             of_copy=round(moved / med / 1e6 / COPY_TB_S, 4)))
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
    spec = importlib.util.spec_from_file_location('kgdet_tool_time_loader', os.path.join(ROOT, 'tools', 'time_loader.py'))
    time_loader = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(time_loader)
    torch.backends.cudnn.benchmark = False
    tmp = tempfile.mkdtemp(prefix='kgdet_draw_')
    spent = dict(draw_s=0.0, encode_thread_s=0.0)
    lock = threading.Lock()
    save_image, draw_call = vz.save_image, vz.DeviceDrawer.__call__

    def timed_save(*a, **kw):
        t0 = time.perf_counter()
        try:
            return save_image(*a, **kw)
        finally:
            with lock:
                spent['encode_thread_s'] += time.perf_counter() - t0

    def timed_draw(self, *a, **kw):
        t0 = time.perf_counter()
        try:
            return draw_call(self, *a, **kw)
        finally:
            spent['draw_s'] += time.perf_counter() - t0
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

        def run(show_dir):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.autocast('cuda', dtype=torch.bfloat16):
                rn.single_gpu_test(model, data, imgs_per_gpu=8, device_preprocess=True, device_results=True, workers=args.workers,
                                   show_dir=show_dir, show_score_thr=args.show_score_thr).release()
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        run(None)                                        # every shape of the set once
        vz.save_image, vz.DeviceDrawer.__call__ = timed_save, timed_draw
        out = dict(images=args.images, workers=args.workers, show_score_thr=args.show_score_thr, plain_s=[], show_s=[], draw_s=[],
                   encode_thread_s=[], cpus_usable=len(os.sched_getaffinity(0)))
        for k in range(2):
            out['plain_s'].append(round(run(None), 3))
            spent.update(draw_s=0.0, encode_thread_s=0.0)
            out['show_s'].append(round(run(os.path.join(tmp, 'shown%d' % k)), 3))
            out['draw_s'].append(round(spent['draw_s'], 3))
            out['encode_thread_s'].append(round(spent['encode_thread_s'], 3))
            out['pictures'] = len(os.listdir(os.path.join(tmp, 'shown%d' % k)))
            print('round %d: %s' % (k, json.dumps(out)), file=sys.stderr, flush=True)
        return out
    finally:
        vz.save_image, vz.DeviceDrawer.__call__ = save_image, draw_call
        shutil.rmtree(tmp, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--sizes', default='624x468,800x1088', help='H x W, comma separated')
    ap.add_argument('--rows', type=int, default=100)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--loop', action='store_true')
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--workers', type=int, default=4)
    ap.add_argument('--show-score-thr', type=float, default=0.3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_draw.py needs a GPU')
    out = dict(loop=loop_legs(args)) if args.loop else dict(kernel=kernel_legs(args))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
