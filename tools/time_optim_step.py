"""Time of the gradient clip + SGD step over the parameter lists of the two detectors, on the GPU, without a forward pass.

Three routes over the same tensors (random gradients, momentum buffers in place), the clip inactive and active:
  (a) clip_grad_norm_ + torch.optim.SGD as runner.build_optimizer constructs it (foreach)
  (b) the same with fused=True
  (c) kgdet_amd.optim.FusedClipSGD (csrc/optim.hip: multi_sqnorm + multi_clip_sgd)
Per route: median / min / max over WINDOWS windows of STEPS steps between two device events (the routes take turns window by
window), kernel launches per step (torch.profiler), and for (c) the achieved bytes/s from the bytes the algorithm moves: the norm
pass reads 4 B per element, the update reads 12 B and writes 8 B (+ 4 B, the scaled gradient, when the clip is active).

"Active" uses max_norm = 1e-7: clip_grad_norm_ scales the gradients in place, so with any ordinary max_norm the second step of a
timing loop would find them at the limit already; below the 1e-6 of the coefficient's denominator the coefficient is < 0.1 whatever
the norm, and the clip stays active in every step (the kernels' time does not depend on the values).

    python tools/time_optim_step.py [--out FILE.json] [--steps 200] [--windows 9]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

COPY_CEILING_TBS = 6.29          # float4 copy measured on the MI355X (HBM3E: 8.0 TB/s by specification)


def parameter_shapes(name):
    from kgdet_amd import build_detector, configs
    cfg = configs.kgdet_r50_fpn() if name == 'kgdet_r50_fpn' else configs.reppoints_kp_r50_fpn()
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    return [tuple(p.shape) for p in model.parameters() if p.requires_grad]


class Route(object):
    def __init__(self, kind, shapes, max_norm, seed=0):
        from kgdet_amd.optim import FusedClipSGD
        g = torch.Generator(device='cuda').manual_seed(seed)
        self.params = [torch.nn.Parameter(torch.randn(s, device='cuda', generator=g) * 0.05) for s in shapes]
        for p in self.params:
            p.grad = torch.randn(p.shape, device='cuda', generator=g) * 1e-3
        kw = dict(fused=True) if kind == 'b' else {}
        self.opt = torch.optim.SGD(self.params, lr=5e-3, momentum=0.9, weight_decay=1e-4, **kw)
        self.clip = dict(max_norm=max_norm, norm_type=2)
        self.kind = kind
        self.opt.step()                                   # creates the momentum buffers
        self.fused = FusedClipSGD() if kind == 'c' else None
        if self.fused is not None and not self.fused.applicable(self.opt, self.params, self.clip):
            raise RuntimeError('the fused clip + SGD step does not apply to this optimizer')

    def step(self):
        if self.fused is not None:
            self.fused.step(self.opt, self.params, self.clip)
        else:
            torch.nn.utils.clip_grad_norm_(self.params, **self.clip)
            self.opt.step()

    def window(self, steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            self.step()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / steps                  # ms per step

    def launches(self, steps=4):
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(steps):
                self.step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
        return n / steps


def measure(name, steps, windows, warmup):
    shapes = parameter_shapes(name)
    numel = sum(int(torch.Size(s).numel()) for s in shapes)
    rows = []
    for label, max_norm in (('inactive', 1e30), ('active', 1e-7)):
        routes = {k: Route(k, shapes, max_norm) for k in 'abc'}
        for r in routes.values():
            for _ in range(warmup):
                r.step()
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(windows):
            for k, r in routes.items():                   # the routes take turns: drift of the machine hits all three alike
                times[k].append(r.window(steps))
        for k, r in routes.items():
            try:
                launches = r.launches()
            except Exception as e:                        # (the profiler is the only source of this number)
                launches = 'not measured (%s)' % type(e).__name__
            med = statistics.median(times[k])
            row = dict(model=name, tensors=len(shapes), elements=numel, clip=label, route=k, ms_median=round(med, 4),
                       ms_min=round(min(times[k]), 4), ms_max=round(max(times[k]), 4), launches_per_step=launches)
            if k == 'c':
                nbytes = numel * (4 + 12 + 8 + (4 if label == 'active' else 0))
                row['bytes_per_step'] = nbytes
                row['achieved_TBps'] = round(nbytes / (med * 1e-3) / 1e12, 3)
                row['share_of_float4_copy_ceiling'] = round(row['achieved_TBps'] / COPY_CEILING_TBS, 3)
            rows.append(row)
        del routes
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_optim_step.py measures on the GPU: none found')
    rows = []
    for name in ('kgdet_r50_fpn', 'reppoints_kp_r50_fpn'):
        rows += measure(name, args.steps, args.windows, args.warmup)
    result = dict(device=torch.cuda.get_device_name(0), steps_per_window=args.steps, windows=args.windows, rows=rows)
    print('| model | clip | route | ms / step (median, min .. max) | launches / step | TB/s |')
    print('|---|---|---|---|---|---|')
    for r in rows:
        print('| %s | %s | %s | %.3f (%.3f .. %.3f) | %s | %s |' % (r['model'], r['clip'], r['route'], r['ms_median'], r['ms_min'],
                                                                     r['ms_max'], r['launches_per_step'], r.get('achieved_TBps', '')))
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
