"""Time ``--json_out``: the host route (``evaluation.results2json`` of the list) against the device route
(``evaluation_device.write_device_results_json`` of the rows in device memory) on the same detections.

    python tools/time_json_out.py [--images N] [--dets D] [--no-host] [--out-dir DIR] [--chunk-mib M]

One synthetic detector-shaped result set as tools/time_eval.py builds it (per image D detections: jittered ground truths of
the committed demo annotations and false positives, float32 boxes, scores and 882 landmark values), once as the list
``single_gpu_test`` returns and once as the ``[N, D, 889]`` device tensor of a ``device_results=True`` run.  At most 2048
distinct images are built; beyond that the set repeats them under fresh image ids.  Both routes write ``P.bbox.json`` and
``P.keypoints.json``, alternating twice (host, device, host, device); after every device run the files are compared with the
host route's (``filecmp.cmp(..., shallow=False)``).  ``--no-host``: the device route alone, twice, nothing to compare with.
The files go to ``--out-dir`` (default: a fresh temporary directory, removed afterwards); the run is refused when the
directory's file system has less free space than the files need.
Prints one JSON line: per run the seconds in total and the bytes written; for a device run also the split -- order + measure
+ scans + the one read-back (``order_measure_s``), the write kernels and the copies (event-timed sums; they overlap the file
writes), the ``f.write`` calls -- and the write kernels' bytes per second."""
import argparse
import filecmp
import importlib.util
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgdet_amd import evaluation as ev  # noqa: E402
from kgdet_amd import evaluation_device as evd  # noqa: E402

DISTINCT = 2048
BYTES_PER_DET = 8900          # text of one detection in both files, rounded up (for the free-space check)


def _time_eval():
    spec = importlib.util.spec_from_file_location('kgdet_tool_time_eval', os.path.join(ROOT, 'tools', 'time_eval.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


class Dataset(object):
    """all the result writers read of a dataset: no annotations"""

    def __init__(self, img_ids, cat_ids):
        self.img_ids, self.cat_ids = list(img_ids), list(cat_ids)

    def __len__(self):
        return len(self.img_ids)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--dets', type=int, default=100)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out-dir', default=None)
    ap.add_argument('--chunk-mib', type=int, default=None, help='chunk_bytes of the device route in MiB (default: its own)')
    args = ap.parse_args(argv)
    import torch
    from kgdet_amd.runner import DeviceResults
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_json_out.py needs a GPU')
    out_dir = args.out_dir or tempfile.mkdtemp(prefix='kgdet_json_out_')
    os.makedirs(out_dir, exist_ok=True)
    need = args.images * args.dets * BYTES_PER_DET * (1 if args.no_host else 2)
    free = shutil.disk_usage(out_dir).free
    if free < need + (1 << 30):
        raise SystemExit('%s has %.1f GB free; the files need about %.1f GB' % (out_dir, free / 1e9, need / 1e9))
    clock = time.perf_counter
    t0 = clock()
    n_built = min(args.images, DISTINCT)
    built = torch.empty((n_built, args.dets, 7 + 882), dtype=torch.float32).pin_memory()

    def rows_out(n, det, label, kpt):
        block = built[n].numpy()
        block[:, :5], block[:, 5], block[:, 6], block[:, 7:] = det, label, len(det), kpt

    gt, results = _time_eval().build(n_built, args.dets, rows_out=rows_out)
    data = Dataset(range(1, args.images + 1), [c['id'] for c in gt['categories']])
    rows = torch.empty((args.images,) + tuple(built.shape[1:]), dtype=torch.float32, device='cuda')
    for n in range(0, args.images, n_built):
        rows[n:n + n_built].copy_(built[:min(n_built, args.images - n)])
    results = [results[n % n_built] for n in range(args.images)] if not args.no_host else None
    del built
    dev = DeviceResults(rows, len(data.cat_ids) + 1)
    out = dict(images=args.images, dets_per_image=args.dets, build_s=round(clock() - t0, 3), out_dir=out_dir, runs=[])
    kw = {} if args.chunk_mib is None else dict(chunk_bytes=args.chunk_mib << 20)
    out['chunk_bytes'] = kw.get('chunk_bytes', evd.JSON_CHUNK_BYTES)
    evd.write_device_results_json(Dataset([1], data.cat_ids), DeviceResults(rows[:1].clone(), dev.num_classes),
                                  os.path.join(out_dir, 'first'))            # context, library load, first launches
    torch.cuda.synchronize()
    host_files = None
    try:
        for k in range(2):
            if not args.no_host:
                t0 = clock()
                host_files = ev.results2json(data, results, os.path.join(out_dir, 'host'))
                out['runs'].append(dict(route='host', total_s=clock() - t0,
                                        bytes=sum(os.path.getsize(host_files[t]) for t in ('bbox', 'keypoints'))))
            timings = {}
            t0 = clock()
            files = evd.write_device_results_json(data, dev, os.path.join(out_dir, 'device'), timings=timings, **kw)
            run = dict(route='device', total_s=clock() - t0)
            run.update(timings)
            run['kernel_bytes_per_s'] = timings['bytes'] / timings['kernel_s'] if timings['kernel_s'] else None
            out['runs'].append(run)
            if host_files is not None:
                for t in ('bbox', 'keypoints'):
                    assert filecmp.cmp(files[t], host_files[t], shallow=False), 'the %s files differ' % t
                out['files_equal'] = True
            for t in ('bbox', 'keypoints'):                         # (the next run's temporary files would double the space)
                os.remove(files[t])
            print('run %d done' % k, file=sys.stderr, flush=True)
    finally:
        for name in os.listdir(out_dir):
            if name.split('.')[0] in ('host', 'device', 'first') and name.endswith('.json'):
                os.remove(os.path.join(out_dir, name))
        if args.out_dir is None:
            shutil.rmtree(out_dir, ignore_errors=True)
    host = [r['total_s'] for r in out['runs'] if r['route'] == 'host']
    device = [r['total_s'] for r in out['runs'] if r['route'] == 'device']
    if host:
        # accepted: both device runs below the host route's faster run by more than the host route's own spread
        out['host_spread_s'] = max(host) - min(host)
        out['accepted'] = bool(min(host) - max(device) > out['host_spread_s'])
        out['ratio'] = min(host) / max(device)

    def tidy(v):
        if isinstance(v, dict):
            return {k: tidy(x) for k, x in v.items()}
        if isinstance(v, list):
            return [tidy(x) for x in v]
        return float('%.4g' % v) if isinstance(v, float) else v
    print(json.dumps(tidy(out)))


if __name__ == '__main__':
    main()
