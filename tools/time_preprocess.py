"""Cost of the input transform, host path against device path, on demo images at img_scale (1333, 800).  Prints one JSON line.

Steps, each a child process under its own ``timeout``, run in order; the first one that fails ends the run (no retries):

* ``transform`` -- in ONE process, alternating per repetition: the host ``datasets.ImageTransform`` per image with 1 and
  with 16 torch threads (the default input path), and ``preprocess.DeviceImageTransform`` at batch 8 and
  batch 1: the upload of the raw bytes alone (host clock ending in a synchronise), the kernel alone (device events over
  ``--inner`` back-to-back launches of a prebuilt job table on device-resident sources) and the whole call from host
  tensors (host clock ending in a synchronise).  The kernel's algorithmic bytes (source bytes + 3 * out_h * out_w * 4 per
  image, from shapes) over its time give the achieved bytes/s and its share of the HBM rate; the kernel streams, so this
  is its bound.
* ``end_to_end`` -- ``runner.single_gpu_test`` images/s over the 32 demo images at ``imgs_per_gpu=8`` with and without
  ``device_preprocess`` (alternated), and with flip TTA.
* ``kernel_trace`` -- one ``rocprofv3 --kernel-trace --stats`` pass of a loop of batch-8 launches, in a run of its own.

python tools/time_preprocess.py [--reps 10] [--inner 50] [--skip-trace]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = (1333, 800)
HBM_MEASURED = 6.29e12       # float4 copy on the MI355X
HBM_SPEC = 8.0e12


def _median(xs):
    import numpy as np
    return float(np.median(xs))


def _setup(batch):
    import torch
    from tests.golden import demo_cases
    data = demo_cases.demo_dataset(test_mode=True)
    same = [i for i, info in enumerate(data.img_infos) if (info['height'], info['width']) in ((624, 468), (960, 640))]
    by = {}
    for i in same:
        by.setdefault((data.img_infos[i]['height'], data.img_infos[i]['width']), []).append(i)
    idx = max(by.values(), key=len)
    raws = [torch.from_numpy(data.load_image(idx[k % len(idx)]).copy()) for k in range(batch)]     # one pad shape
    return data, raws


def step_transform(a):
    import torch
    from kgdet_amd import datasets
    assert torch.cuda.is_available(), 'time_preprocess.py measures the GPU'
    out = {}
    data, raws8 = _setup(8)
    T = data.device_transform()
    host = datasets.ImageTransform(size_divisor=data.size_divisor, **data.img_norm_cfg)
    arrays = [r.numpy() for r in raws8]
    out['source_hw'] = list(raws8[0].shape[:2])

    def cpu_ms(threads):
        torch.set_num_threads(threads)
        t0 = time.perf_counter()
        for arr in arrays:
            host(arr, SCALE)
        return (time.perf_counter() - t0) * 1e3 / len(arrays)

    def device_case(raws):
        B = len(raws)
        scales, flips = [SCALE] * B, [False] * B
        plans = [T.plan(r, SCALE) for r in raws]
        H, W = plans[0][3][:2]
        dst = torch.empty((B, 3, H, W), dtype=torch.float32, device='cuda')
        dev = [r.cuda() for r in raws]
        tables = T.job_tables(dev, plans, flips, [dst[b] for b in range(B)])
        byts = sum(r.numel() for r in raws) + B * 3 * H * W * 4
        raw_bytes = sum(r.numel() for r in raws)

        def upload():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            T._upload(raws)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def kernel():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            T.launch_tables(tables)
            e0.record()
            for _ in range(a.inner):
                T.launch_tables(tables)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.inner

        def whole():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            T(raws, scales, flips, out=dst)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        return dict(B=B, out_hw=[H, W], bytes=byts, raw_bytes=raw_bytes, float_bytes=B * 3 * H * W * 4, upload=upload,
                    kernel=kernel, whole=whole)

    cases = {'batch8': device_case(raws8), 'batch1': device_case(raws8[:1])}
    acc = {'cpu_1t': [], 'cpu_16t': []}
    for name in cases:
        for k in ('upload', 'kernel', 'whole'):
            acc[name + '_' + k] = []
    for rep in range(a.warmup + a.reps):
        row = {'cpu_1t': cpu_ms(1)}
        for k in ('upload', 'kernel', 'whole'):
            row['batch8_' + k] = cases['batch8'][k]()
        row['cpu_16t'] = cpu_ms(16)
        for k in ('upload', 'kernel', 'whole'):
            row['batch1_' + k] = cases['batch1'][k]()
        if rep >= a.warmup:
            for k, v in row.items():
                acc[k].append(v)
    out['cpu_transform_ms_per_image'] = {'threads_1': round(_median(acc['cpu_1t']), 3), 'threads_16': round(_median(acc['cpu_16t']), 3),
                                         'threads_16_min': round(min(acc['cpu_16t']), 3)}
    for name, c in cases.items():
        B = c['B']
        k_ms = _median(acc[name + '_kernel'])
        rec = {'out_hw': c['out_hw'], 'raw_bytes': c['raw_bytes'], 'float_bytes': c['float_bytes'],
               'upload_ms_per_image': round(_median(acc[name + '_upload']) / B, 4),
               'kernel_us_per_image': round(k_ms * 1e3 / B, 2), 'kernel_us_per_launch': round(k_ms * 1e3, 2),
               'whole_call_ms_per_image': round(_median(acc[name + '_whole']) / B, 4),
               'whole_call_ms_per_image_max': round(max(acc[name + '_whole']) / B, 4),
               'kernel_algorithmic_bytes': c['bytes'], 'kernel_bytes_per_s': round(c['bytes'] / (k_ms * 1e-3), 0)}
        rec['share_of_hbm_measured_6.29TBps'] = round(rec['kernel_bytes_per_s'] / HBM_MEASURED, 4)
        rec['share_of_hbm_spec_8TBps'] = round(rec['kernel_bytes_per_s'] / HBM_SPEC, 4)
        rec['bound'] = 'bandwidth'
        rec['speedup_vs_cpu_16t_upload_included'] = round(out['cpu_transform_ms_per_image']['threads_16']
                                                          / (_median(acc[name + '_whole']) / B), 1)
        out[name] = rec
    # the float batch the host path has to copy instead of the raw bytes
    img = torch.empty((8, 3) + tuple(cases['batch8']['out_hw']), dtype=torch.float32).pin_memory()
    ts = []
    for _ in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img.cuda(non_blocking=True)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    out['host_path_float_upload_ms_per_image_pinned'] = round(_median(ts[a.warmup:]) / 8, 4)
    print(json.dumps(out))


def step_end_to_end(a):
    import torch
    from kgdet_amd import runner
    from tests.golden import demo_cases
    assert torch.cuda.is_available(), 'time_preprocess.py measures the GPU'
    _, model = demo_cases.demo_detector()
    model = model.cuda().eval()
    to_dev = lambda t: t.cuda(non_blocking=True)
    torch.set_num_threads(16)
    out = {}

    def rate(device_preprocess, ipg, **kw):
        data = demo_cases.demo_dataset(test_mode=True, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = runner.single_gpu_test(model, data, to_device=to_dev, imgs_per_gpu=ipg, device_preprocess=device_preprocess)
        torch.cuda.synchronize()
        return len(res) / (time.perf_counter() - t0)

    for name, ipg, kw in (('imgs_per_gpu_8', 8, {}), ('flip_tta', 1, dict(flip_ratio=0.5))):
        rate(False, ipg, **kw), rate(True, ipg, **kw)                     # every shape warmed on both paths
        host, dev = [], []
        for _ in range(a.e2e_reps):
            host.append(rate(False, ipg, **kw))
            dev.append(rate(True, ipg, **kw))
        out[name] = {'host_transform_img_per_s': round(_median(host), 1), 'device_preprocess_img_per_s': round(_median(dev), 1),
                     'host_all': [round(x, 1) for x in host], 'device_all': [round(x, 1) for x in dev]}
    out['note'] = 'demo images are rendered in the loop (no JPEG decode); host transform with 16 torch threads'
    print(json.dumps(out))


def step_kernel_loop(a):
    import torch
    data, raws = _setup(8)
    T = data.device_transform()
    plans = [T.plan(r, SCALE) for r in raws]
    H, W = plans[0][3][:2]
    dst = torch.empty((8, 3, H, W), dtype=torch.float32, device='cuda')
    tables = T.job_tables([r.cuda() for r in raws], plans, [False] * 8, [dst[b] for b in range(8)])
    for _ in range(a.inner + 5):
        T.launch_tables(tables)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--e2e-reps', type=int, default=2)
    ap.add_argument('--skip-trace', action='store_true')
    ap.add_argument('--trace-dir', default=None)
    ap.add_argument('--step', default=None, choices=['transform', 'end_to_end', 'kernel_loop'])
    a = ap.parse_args()
    if a.step is not None:
        return {'transform': step_transform, 'end_to_end': step_end_to_end, 'kernel_loop': step_kernel_loop}[a.step](a)

    me = [sys.executable, os.path.abspath(__file__), '--reps', str(a.reps), '--warmup', str(a.warmup), '--inner', str(a.inner),
          '--e2e-reps', str(a.e2e_reps)]
    out = {}

    def child(name, limit, cmd):
        """one step under its own time limit; a failure ends the run (nothing more is started on the GPU)"""
        p = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            out['failed_step'] = {'name': name, 'returncode': p.returncode}
            print(json.dumps(out))
            sys.exit(1)
        return p.stdout

    out['transform'] = json.loads(child('transform', 300, me + ['--step', 'transform']).strip().splitlines()[-1])
    out['end_to_end'] = json.loads(child('end_to_end', 420, me + ['--step', 'end_to_end']).strip().splitlines()[-1])
    if not a.skip_trace:
        trace_dir = a.trace_dir or tempfile.mkdtemp(prefix='time_preprocess_')
        child('kernel_trace', 300, ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', trace_dir, '-o',
                                    'pre', '--'] + me + ['--step', 'kernel_loop'])
        rows = []
        for path in glob.glob(os.path.join(trace_dir, '**', '*kernel_stats.csv'), recursive=True):
            rows += [r for r in csv.DictReader(open(path)) if 'image_preprocess_kernel' in r['Name']]
        if not rows:
            out['failed_step'] = {'name': 'kernel_trace', 'returncode': 'no image_preprocess_kernel row in the stats'}
            print(json.dumps(out))
            sys.exit(1)
        r = rows[0]
        out['kernel_trace_batch8'] = {'calls': int(r['Calls']), 'average_us': round(float(r['AverageNs']) / 1e3, 2),
                                      'min_us': round(float(r['MinNs']) / 1e3, 2), 'max_us': round(float(r['MaxNs']) / 1e3, 2)}
        byts = out['transform']['batch8']['kernel_algorithmic_bytes']
        bps = byts / (float(r['AverageNs']) * 1e-9)
        out['kernel_trace_batch8'].update(bytes_per_s=round(bps, 0), share_of_hbm_measured=round(bps / HBM_MEASURED, 4))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
