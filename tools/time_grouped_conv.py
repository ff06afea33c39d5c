"""Time the grouped 3x3 convolutions of a ResNeXt's conv2 (kgdet_amd/grouped_conv.py, csrc/grouped_conv.hip) against torch's
route (``F.conv2d(groups=)`` and ``aten.convolution_backward``: MIOpen), alternated in one process.

    python tools/time_grouped_conv.py [--nets 32x4d,64x4d] [--batch 2] [--size 800x1344] [--windows 9] [--iters 20] [--step]

Shapes: the distinct conv2 shapes of ResNeXt-101 at the given batch and image size -- the maps of layers 1-4 (image / 4 .. / 32)
at 4, 8, 16 and 32 channels per group, stride 1, and the three stride-2 entries at the head of layers 2-4 -- with the number of
layers of each shape.  Forward, grad_input and grad_weight are timed each on its own: ``--windows`` windows of ``--iters`` calls
between two events per route, the two routes taking turns window by window; median, min and max in microseconds, the bytes a call
must move (its operands and its result once) and that traffic as a share of the 6.29 TB/s of a float4 copy.  ``--step``: one
eager KGDet training step on the X101-32x4d model with every class on the route, with the default classes and with every
class on torch, in turn, twice (``--nets ''`` skips the kernel table).  Prints a table and one JSON line.

    python tools/time_grouped_conv.py --bf16 [--nets 32x4d,64x4d] [--batch 8] [--size 800x1344] [--step]

``--bf16``: the inference route on channels-last bf16 storage (csrc/grouped_conv_nhwc.hip) at batch 8 by default.  Per shape the
raw convolution -- ``F.conv2d`` against ``grouped_conv.conv3x3_nhwc`` -- and the convolution with shift and ReLU -- ``F.conv2d``
+ ``kgdet_bias_act`` against the route's one launch --, the routes taking turns in the same windows; the verdict per
(channels per group, stride) class: faster only where the gap between the medians exceeds the spread (max - min) of both
routes' windows, in both modes.  ``--bf16 --step``: one bf16 autocast ``simple_test`` of the X101-32x4d detector at that batch
with the switch off, at ``force`` and at ``1``, in turn, twice.
A run without a GPU fails."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TB_S = 6.29
BLOCKS = (3, 4, 23, 3)       # ResNeXt-101


def shapes(net, batch, H, W):
    """[(label, layers, B, C, cpg, H, W, stride)] of conv2 in a ResNeXt-101 <groups>x<base_width>d on a [B, 3, H, W] batch"""
    groups, base_width = (int(v) for v in net.rstrip('d').split('x'))
    out, h, w = [], (H + 3) // 4, (W + 3) // 4
    for stage, blocks in enumerate(BLOCKS):
        width = (64 << stage) * base_width // 64 * groups
        cpg = width // groups
        if stage:
            out.append(('layer%d.0' % (stage + 1), 1, batch, width, cpg, h, w, 2))
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        out.append(('layer%d' % (stage + 1), blocks - (1 if stage else 0), batch, width, cpg, h, w, 1))
    return out


def stats(values):
    return dict(median=round(float(np.median(values)), 1), min=round(float(min(values)), 1), max=round(float(max(values)), 1))


def window(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def alternate(fns, windows, iters):
    """{name: [us per call] per window}: every route warmed up, then one window each in turn"""
    import torch
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            out[k].append(window(fn, iters))
    return out


def time_shape(B, C, cpg, H, W, stride, windows, iters):
    import torch
    import torch.nn.functional as F
    from kgdet_amd import grouped_conv as G
    groups = C // cpg
    g = torch.Generator('cuda').manual_seed(C + H)
    x = torch.randn(B, C, H, W, device='cuda', generator=g)
    w = torch.randn(C, cpg, 3, 3, device='cuda', generator=g) * 0.05
    y = F.conv2d(x, w, None, stride, 1, 1, groups)
    gy = torch.randn(y.shape, device='cuda', generator=g)
    assert G.shape_ok(x.shape, w.shape, stride, 1, 1, groups)
    back = torch.ops.aten.convolution_backward

    def torch_back(mask):
        return back(gy, x, w, None, [stride, stride], [1, 1], [1, 1], False, [0, 0], groups, mask)
    legs = {
        'forward': ({'hip': lambda: G.forward(x, w, stride), 'torch': lambda: F.conv2d(x, w, None, stride, 1, 1, groups)},
                    x.numel() + y.numel() + w.numel()),
        'grad_input': ({'hip': lambda: G.grad_input(gy, w, x.shape, stride), 'torch': lambda: torch_back([True, False, False])},
                       x.numel() + y.numel() + w.numel()),
        'grad_weight': ({'hip': lambda: G.grad_weight(gy, x, w, stride), 'torch': lambda: torch_back([False, True, False])},
                        x.numel() + y.numel() + w.numel())}
    # the two routes agree (fp32 sums in another order) before anything is timed
    for got, want in ((G.forward(x, w, stride), y), (G.grad_input(gy, w, x.shape, stride), torch_back([True, False, False])[0]),
                      (G.grad_weight(gy, x, w, stride), torch_back([False, True, False])[1])):
        assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max())
    rec = {}
    for name, (fns, floats) in legs.items():
        t = alternate(fns, windows, iters)
        nbytes = 4 * floats
        rec[name] = dict(bytes=nbytes, hip_us=stats(t['hip']), torch_us=stats(t['torch']),
                         hip_share_of_copy=round(nbytes / (np.median(t['hip']) * 1e-6) / (COPY_TB_S * 1e12), 3),
                         torch_share_of_copy=round(nbytes / (np.median(t['torch']) * 1e-6) / (COPY_TB_S * 1e12), 3),
                         hip_over_torch=round(float(np.median(t['hip']) / np.median(t['torch'])), 3))
    return rec


def time_shape_bf16(B, C, cpg, H, W, stride, windows, iters):
    import torch
    import torch.nn.functional as F
    from kgdet_amd import backbone, grouped_conv as G
    groups = C // cpg
    g = torch.Generator('cuda').manual_seed(C + H)
    cl = torch.channels_last
    x = torch.randn(B, C, H, W, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=cl)
    w = (torch.randn(C, cpg, 3, 3, device='cuda', generator=g) * 0.05).to(torch.bfloat16).contiguous(memory_format=cl)
    bias = torch.randn(C, device='cuda', generator=g)
    assert G.shape_ok(x.shape, w.shape, stride, 1, 1, groups) and C % 8 == 0

    def torch_raw():
        return F.conv2d(x, w, None, stride, 1, 1, groups)
    legs = {
        'raw': {'hip': lambda: G.conv3x3_nhwc(x, w, stride), 'torch': torch_raw},
        'bias_relu': {'hip': lambda: G.conv3x3_nhwc(x, w, stride, bias, True),
                      'torch': lambda: backbone._epilogue_(torch_raw(), bias, None, True)}}
    y = torch_raw()
    assert y.is_contiguous(memory_format=cl)
    # the two routes agree (fp32 sums in another order, one bf16 rounding apart at the most) before anything is timed
    for name, fns in legs.items():
        got, want = fns['hip']().float(), fns['torch']().float()
        assert float((got - want).abs().max()) <= 2.0 ** -6 * float(want.abs().max()), name
    nbytes = 2 * (x.numel() + y.numel() + w.numel())
    rec = {}
    with torch.no_grad():
        for name, fns in legs.items():
            t = alternate(fns, windows, iters)
            hip, ref = stats(t['hip']), stats(t['torch'])
            spread = max(hip['max'] - hip['min'], ref['max'] - ref['min'])
            rec[name] = dict(bytes=nbytes, hip_us=hip, torch_us=ref,
                             hip_share_of_copy=round(nbytes / (np.median(t['hip']) * 1e-6) / (COPY_TB_S * 1e12), 3),
                             torch_share_of_copy=round(nbytes / (np.median(t['torch']) * 1e-6) / (COPY_TB_S * 1e12), 3),
                             hip_over_torch=round(float(np.median(t['hip']) / np.median(t['torch'])), 3),
                             faster=bool(ref['median'] - hip['median'] > spread))
    return rec


def time_step_bf16(batch, H, W, rounds=2, iters=3):
    """one bf16 autocast simple_test of the X101-32x4d KGDet model, switch off / force / 1 alternated ``rounds`` times: ms"""
    import torch
    from kgdet_amd import configs, grouped_conv as G, synthetic
    from kgdet_amd.registry import build_detector
    cfg = configs.kgdet_x101_fpn()
    torch.manual_seed(0)
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda()
    model.eval()
    data = synthetic.make_batch(batch, 'cuda', seed=0, img_shape=(H, W, 3), pad_shape=(H, W, 3))
    auto = lambda: torch.autocast('cuda', dtype=torch.bfloat16)       # noqa: E731
    synthetic.calibrate_scores(model, data, cfg.test_cfg.score_thr, autocast=auto())

    def step():
        with torch.no_grad(), auto():
            model.simple_test(data['img'], data['img_meta'], rescale=True)
    legs = ('0', 'force', '1')
    out = {name: [] for name in legs}
    saved = G.BF16
    try:
        for G.BF16 in legs:          # warm-up of every route (the measured 1x1 choices, MIOpen's algorithms)
            for _ in range(3):
                step()
        for _ in range(rounds):
            for G.BF16 in legs:
                G.reset_calls_nhwc()
                out[G.BF16].append(window(step, iters) / 1000.0)
                assert (sum(G.calls_nhwc.values()) > 0) == (G.BF16 == 'force' or (G.BF16 == '1' and len(G.TORCH_CLASSES_BF16) < 8))
    finally:
        G.BF16 = saved
    return {k: [round(v, 2) for v in vs] for k, vs in out.items()}


def main_bf16(args, H, W):
    batch = 8 if args.batch is None else args.batch
    result = dict(bf16=True, batch=batch, size=[H, W], windows=args.windows, iters=args.iters, nets={})
    verdict = {}
    for net in [n for n in args.nets.split(',') if n]:
        rows = []
        for label, layers, B, C, cpg, h, w, stride in shapes(net, batch, H, W):
            rec = time_shape_bf16(B, C, cpg, h, w, stride, args.windows, args.iters)
            rows.append(dict(layer=label, layers=layers, C=C, cpg=cpg, H=h, W=w, stride=stride, **rec))
            for name in ('raw', 'bias_relu'):
                r = rec[name]
                verdict.setdefault((cpg, stride), []).append(r['faster'])
                print('%-6s %-9s x%-2d C=%4d cpg=%2d %3dx%-3d s%d %-9s hip %8.1f us (%.1f-%.1f, %.2f of copy)  torch %8.1f us '
                      '(%.1f-%.1f, %.2f of copy)  hip/torch %.2f %s' % (
                          net, label, layers, C, cpg, h, w, stride, name, r['hip_us']['median'], r['hip_us']['min'],
                          r['hip_us']['max'], r['hip_share_of_copy'], r['torch_us']['median'], r['torch_us']['min'],
                          r['torch_us']['max'], r['torch_share_of_copy'], r['hip_over_torch'],
                          'faster' if r['faster'] else 'not faster'), flush=True)
        result['nets'][net] = rows
    result['torch_classes'] = sorted(k for k, v in verdict.items() if not all(v))
    print('classes that stay on torch (not faster beyond the spread in every row):', result['torch_classes'], flush=True)
    if args.step:
        result['step_ms'] = time_step_bf16(batch, H, W)
        print('bf16 simple_test, ms:', result['step_ms'], flush=True)
    print(json.dumps(result))


def time_step(batch, H, W, rounds=2, iters=3):
    """one eager training step of the X101-32x4d KGDet model, route on / off alternated ``rounds`` times: ms per step"""
    import torch
    from kgdet_amd import configs, grouped_conv as G, synthetic
    from kgdet_amd.registry import build_detector
    cfg = configs.kgdet_x101_fpn()
    torch.manual_seed(0)
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda()
    model.train()
    data = synthetic.make_batch(batch, 'cuda', seed=0, img_shape=(H, W, 3), pad_shape=(H, W, 3))

    def step():
        model.zero_grad(set_to_none=True)
        losses = model(data['img'], data['img_meta'], return_loss=True, gt_bboxes=data['gt_bboxes'],
                       gt_labels=data['gt_labels'], gt_keypoints=data['gt_keypoints'])
        sum(sum(v) if isinstance(v, (list, tuple)) else v for k, v in losses.items() if 'loss' in k).backward()
    # every class on the route / the default classes (grouped_conv.TORCH_CLASSES stay on torch) / every class on torch
    legs = (('hip', True, True), ('default', True, False), ('torch', False, False))
    out = {name: [] for name, _, _ in legs}
    saved = (G.ENABLED, G.FORCE)
    try:
        for _, G.ENABLED, G.FORCE in legs:       # warm-up of every route (MIOpen picks its algorithms in the first calls)
            for _ in range(2):
                step()
        for _ in range(rounds):
            for name, G.ENABLED, G.FORCE in legs:
                G.reset_calls()
                out[name].append(window(step, iters) / 1000.0)
                assert (G.calls['forward'] > 0) == G.ENABLED
    finally:
        G.ENABLED, G.FORCE = saved
    return {k: [round(v, 2) for v in vs] for k, vs in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nets', default='32x4d,64x4d')
    ap.add_argument('--batch', type=int, default=None, help='default 2, with --bf16 8')
    ap.add_argument('--size', default='800x1344')
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--step', action='store_true')
    ap.add_argument('--bf16', action='store_true', help='the bf16 channels-last inference route instead of the fp32 kernels')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('time_grouped_conv: needs a GPU (nothing is measured without one)')
    H, W = (int(v) for v in args.size.split('x'))
    if args.bf16:
        return main_bf16(args, H, W)
    args.batch = 2 if args.batch is None else args.batch
    result = dict(batch=args.batch, size=[H, W], windows=args.windows, iters=args.iters, nets={})
    for net in [n for n in args.nets.split(',') if n]:
        rows = []
        for label, layers, B, C, cpg, h, w, stride in shapes(net, args.batch, H, W):
            rec = time_shape(B, C, cpg, h, w, stride, args.windows, args.iters)
            rows.append(dict(layer=label, layers=layers, C=C, cpg=cpg, H=h, W=w, stride=stride, **rec))
            for name in ('forward', 'grad_input', 'grad_weight'):
                r = rec[name]
                print('%-6s %-9s x%-2d C=%4d cpg=%2d %3dx%-3d s%d %-11s hip %8.1f us (%.1f-%.1f, %.2f of copy)  torch %8.1f us '
                      '(%.1f-%.1f)  hip/torch %.2f' % (net, label, layers, C, cpg, h, w, stride, name, r['hip_us']['median'],
                                                       r['hip_us']['min'], r['hip_us']['max'], r['hip_share_of_copy'],
                                                       r['torch_us']['median'], r['torch_us']['min'], r['torch_us']['max'],
                                                       r['hip_over_torch']), flush=True)
        result['nets'][net] = rows
    if args.step:
        result['step_ms'] = time_step(args.batch, H, W)
        print('training step, ms:', result['step_ms'], flush=True)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
