"""Per-image cost of test-time augmentation on the demo KGDet detector, one demo image through the demo test pipeline
at img_scale (1333, 800) (plus (1000, 600) for the second scale; the tensor shapes are printed): simple_test, flip TTA,
two-scale + flip TTA, host clock around work that ends in a device synchronise, median of --reps after --warmup.
Then the merge + NMS alone on the flip-TTA and the 4-augmentation candidates of that image, device events over --inner
back-to-back calls (so: per call, Python wrapper included, not a kernel-trace time): the kgdet_aug_merge kernel
against the pure-torch restatement, and the routed NMS (fused hard NMS for these sizes) against the per-class loop.
Prints one JSON line.  python tools/time_aug_test.py [--reps 20] [--warmup 3] [--inner 50]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--image', type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_aug_test.py measures the GPU'
    from kgdet_amd.detector import merge_aug_results_kp
    from kgdet_amd.postprocess import aug_merge_kp, aug_nms_kp, multiclass_nms_kp, multiclass_nms_fused_supported
    from tests.golden import demo_cases

    _, model = demo_cases.demo_detector()
    model = model.cuda().eval()
    cfg = model.test_cfg
    out = {}

    def sample(**kw):
        data = demo_cases.demo_dataset(test_mode=True, **kw)
        d = data[a.image]
        return [t[None].cuda() for t in d['img']], [[m] for m in d['img_meta']]

    cases = {'simple_test': sample(), 'flip': sample(flip_ratio=0.5),
             'two_scale_flip': sample(flip_ratio=0.5, img_scale=[(1333, 800), (1000, 600)])}
    out['shapes'] = {k: [list(t.shape[2:]) for t in v[0]] for k, v in cases.items()}

    def per_image_ms(imgs, metas):
        ts = []
        for i in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                model(imgs, metas, return_loss=False, rescale=True)
            torch.cuda.synchronize()
            if i >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    for name, (imgs, metas) in cases.items():
        med, lo, hi = per_image_ms(imgs, metas)
        out['%s_ms' % name] = {'median': round(med, 3), 'min': round(lo, 3), 'max': round(hi, 3)}

    def event_us(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return round(e0.elapsed_time(e1) * 1e3 / a.inner, 2)

    for name in ('flip', 'two_scale_flip'):
        imgs, metas = cases[name]
        with torch.no_grad():
            cands = model.aug_candidates(imgs, metas)
        m = [x[0] for x in metas]
        parts = ([c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands], m)
        b, s, k = aug_merge_kp(*parts)
        k = k.reshape(k.shape[0], -1)
        T, C = s.shape[0], s.shape[1] - 1
        moved = sum(x.numel() * 4 for c in cands for x in c) * 2          # every candidate byte read once, written once
        rec = {'augmentations': len(cands), 'candidates': T, 'merge_bytes': moved,
               'fused_nms': multiclass_nms_fused_supported(1, T, C, cfg.max_per_img)}
        rec['merge_kernel_us'] = event_us(lambda: aug_merge_kp(*parts))
        rec['merge_torch_us'] = event_us(lambda: merge_aug_results_kp(*parts))
        # (the routed NMS ends in one host read of the detection count; the per-class loop reads per class)
        rec['nms_routed_us'] = event_us(lambda: aug_nms_kp(b, s, k, cfg))
        rec['nms_per_class_loop_us'] = event_us(lambda: multiclass_nms_kp(b, s, k, cfg.score_thr, cfg.nms, cfg.max_per_img))
        out[name] = rec
    print(json.dumps(out))


if __name__ == '__main__':
    main()
