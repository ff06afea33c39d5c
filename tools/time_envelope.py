"""Time of the whole-model envelope scan (kgdet_amd/numerics.py EnvelopeGuard.check -> csrc/range_scan.hip) on the GPU.

The guard of a config's detector is built once; then WINDOWS windows of STEPS scan launches (no read-back) between two device
events, and separately the wall time of `check()` itself (launch + the one read-back + the host loop over the records).
Reported: rows and elements of the table, bytes read per scan (4 B per scanned element; a conv + BatchNorm pair is scanned
folded AND plain, so backbone weights count twice), median / min / max per scan, bytes/s against the 6.29 TB/s of a float4 copy
on the MI355X, kernel launches per scan (torch.profiler), and the median wall time of `check()`.

    python tools/time_envelope.py [--config kgdet_r50_fpn] [--out FILE.json] [--steps 50] [--windows 9]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

COPY_CEILING_TBS = 6.29          # float4 copy measured on the MI355X (HBM3E: 8.0 TB/s by specification)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='kgdet_r50_fpn', choices=['kgdet_r50_fpn', 'reppoints_kp_r50_fpn'])
    ap.add_argument('--out')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--windows', type=int, default=9)
    args = ap.parse_args()
    from kgdet_amd import build_detector, configs, numerics
    cfg = getattr(configs, args.config)()
    torch.manual_seed(0)
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda()
    guard = numerics.EnvelopeGuard(model)
    table = guard.table()
    elements = sum(l.conv.weight.numel() for l in guard.layers)
    violations = guard.check()                               # (also the warm-up)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            table.launch()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / args.steps)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        table.launch()
        torch.cuda.synchronize()
    launches = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
    walls = []
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        guard.check()
        walls.append((time.perf_counter() - t0) * 1e6)
    med = statistics.median(times)
    res = dict(config=args.config, rows=len(guard.layers), elements=elements, bytes=4 * elements, blocks=table.blocks,
               parameters=sum(p.numel() for p in model.parameters()), violations=len(violations),
               scan_us=dict(median=med, min=min(times), max=max(times)), steps=args.steps, windows=args.windows,
               tbytes_per_s=4 * elements / med / 1e6, fraction_of_copy_ceiling=4 * elements / med / 1e6 / COPY_CEILING_TBS,
               device_launches_per_scan=launches, check_wall_us=statistics.median(walls))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
