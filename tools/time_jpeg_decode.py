"""Time the device JPEG decoder, ``kgdet_jpeg_decode`` (kgdet_amd/jpeg.py: ``DeviceJpegDecoder``), alone.

    python tools/time_jpeg_decode.py [--batches 8,32] [--sizes 624x468,880x1320] [--windows 9] [--iters 10] [--threads 16]
                                     [--sampling {420,422}] [--restart {none,rows,N}] [--entry {baseline,camera,both}]

Per size (H x W) one picture is rendered as the demo set is (blocks of 32 x 32 pixels of one colour under noise of sigma 6),
written by PIL at quality 90 (4:2:0), and -- beside it -- one picture of one colour (white) of the same size.  The files' bytes
lie in device memory; ``--windows`` windows of ``--iters`` calls between two events.  Per leg: the microseconds per image of the
whole call and after each of its four kernels (``kgdet_jpeg_decode_stages`` with 1 .. 4 stages: the differences are the
kernels' own times; median of the windows, min and max), the bytes uploaded per image against the raw route's 3 H W, the back end's bytes
(coefficients read, planes written and read, picture written) against the 6.29 TB/s of a float4 copy, the rounds the fixpoint
took, once the check that the picture equals PIL's, and PIL's decode of the same file on one thread and as wall time per image
on ``--threads`` threads.  ``--sampling 422`` writes the files with PIL's ``subsampling='4:2:2'``; ``--restart rows`` with
``restart_marker_rows=1``, ``--restart N`` with ``restart_marker_blocks=N`` (N MCUs an interval).  ``--entry``: the entry point,
``kgdet_jpeg_decode`` (baseline), ``kgdet_jpeg_decode_camera`` (camera) or both in turn on the same files (a 4:2:2 file or one
with restart intervals only has the camera leg).  ``--threads 0`` leaves PIL's timing out.  Prints one JSON line."""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TB_S = 6.29


def render(H, W, seed=0):
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 256, ((H + 31) // 32, (W + 31) // 32, 3))
    img = np.repeat(np.repeat(blocks, 32, axis=0), 32, axis=1)[:H, :W].astype(np.float64)
    return np.clip(np.rint(img + rng.normal(0, 6, img.shape)), 0, 255).astype(np.uint8)


def write(img, sampling='420', restart='none'):
    from PIL import Image
    kw = dict(subsampling='4:2:2') if sampling == '422' else {}
    if restart == 'rows':
        kw['restart_marker_rows'] = 1
    elif restart != 'none':
        kw['restart_marker_blocks'] = int(restart)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', quality=90, **kw)
    return buf.getvalue()


def stats(values):
    return dict(median=round(float(np.median(values)), 2), min=round(float(min(values)), 2), max=round(float(max(values)), 2))


def time_calls(fn, windows, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / iters)
    return out


def leg(data, batch, windows, iters, threads, camera=False):
    import torch
    from kgdet_amd import jpeg
    frame = jpeg.parse_header(data, camera)
    H, W = frame['H'], frame['W']
    files, frames = [data] * batch, [frame] * batch
    total, places = jpeg.pack_files(files, frames)
    host = np.zeros(total, dtype=np.uint8)
    jpeg.pack_files(files, frames, host)
    src = torch.from_numpy(host).cuda()
    jobs = [(so, sb, to, H, W, frame['mode'], frame.get('restart_interval', 0)) for so, sb, to in places]
    decoder = jpeg.DeviceJpegDecoder(camera=camera)
    out = torch.empty(batch * ((3 * H * W + 255) // 256 * 256), dtype=torch.uint8, device='cuda')
    images, status = decoder.decode(src, jobs, out)
    ref = jpeg.decode_pil(data)
    assert status.cpu().tolist() == [0] * batch and all(np.array_equal(img.cpu().numpy(), ref) for img in images[:2] + images[-1:])
    result = dict(H=H, W=W, batch=batch, entry='camera' if camera else 'baseline', restart_interval=frame.get('restart_interval', 0),
                  file_bytes=len(data), uploaded_per_image=total // batch, raw_bytes=3 * H * W,
                  rounds=decoder.rounds(1)[0])
    after = {}
    for k in (1, 2, 3, 4):
        after[k] = [t / batch for t in time_calls(lambda: decoder.decode(src, jobs, out, stages=k), windows, iters)]
    assert decoder.decode(src, jobs, out, stages=2)[1].cpu().tolist() == [-1] * batch     # a call cut short says so
    result['us_per_image'] = stats(after[4])
    names = ('unstuff', 'huffman', 'idct', 'colour')
    result['us_per_image_after'] = {names[k - 1]: stats(after[k]) for k in after}
    result['us_per_image_stage'] = {names[k - 1]: round(float(np.median(after[k]) - (np.median(after[k - 1]) if k > 1 else 0.0)), 2)
                                    for k in after}
    mw, mh, bpm = jpeg.frame_blocks(frame)
    planes = 64 * mw * mh * bpm                      # (4:2:0: 256 + 128 bytes an MCU, 4:2:2: 128 + 128)
    back_bytes = 128 * mw * mh * bpm + 2 * planes + 3 * H * W
    back_us = result['us_per_image_stage']['idct'] + result['us_per_image_stage']['colour']
    result['back_end'] = dict(bytes_per_image=back_bytes, us_per_image=round(back_us, 2),
                              fraction_of_copy=round(back_bytes / (back_us * 1e-6) / (COPY_TB_S * 1e12), 4))
    if threads < 1:
        return result
    t = time.perf_counter()
    for _ in range(8):
        jpeg.decode_pil(data)
    result['pil_us_one_thread'] = round((time.perf_counter() - t) / 8 * 1e6, 1)
    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(jpeg.decode_pil, [data] * threads))
        t = time.perf_counter()
        list(pool.map(jpeg.decode_pil, [data] * (8 * threads)))
        result['pil_us_wall_%d_threads' % threads] = round((time.perf_counter() - t) / (8 * threads) * 1e6, 1)
    return result


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    parser.add_argument('--batches', default='8,32')
    parser.add_argument('--sizes', default='624x468,880x1320')
    parser.add_argument('--windows', type=int, default=9)
    parser.add_argument('--iters', type=int, default=10)
    parser.add_argument('--threads', type=int, default=16)
    parser.add_argument('--sampling', choices=('420', '422'), default='420')
    parser.add_argument('--restart', default='none', help="none, rows (one MCU row an interval) or N (MCUs an interval)")
    parser.add_argument('--entry', choices=('baseline', 'camera', 'both'), default='baseline')
    args = parser.parse_args(argv)
    import torch
    from kgdet_amd import jpeg
    if not (args.restart in ('none', 'rows') or (args.restart.isdigit() and 1 <= int(args.restart) <= 65535)):
        raise SystemExit('--restart is none, rows or an interval of 1 .. 65535 MCUs')
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_jpeg_decode.py needs a GPU')
    legs = []
    for size in args.sizes.split(','):
        H, W = (int(v) for v in size.split('x'))
        for name, img in (('rendered', render(H, W)), ('uniform', np.full((H, W, 3), 255, dtype=np.uint8))):
            data = write(img, args.sampling, args.restart)
            old_takes = not isinstance(jpeg.parse_header(data), str)
            if args.entry == 'baseline' and not old_takes:
                raise SystemExit('kgdet_jpeg_decode does not take these files (%s): --entry camera' % jpeg.parse_header(data))
            for batch in (int(b) for b in args.batches.split(',')):
                if name == 'uniform' and batch != 8:
                    continue
                for camera in (False, True):
                    if args.entry in ('both', 'camera' if camera else 'baseline') and (camera or old_takes):
                        legs.append(dict(leg(data, batch, args.windows, args.iters, min(args.threads, 16), camera), picture=name))
    print(json.dumps(dict(tool='time_jpeg_decode', legs=legs)))


if __name__ == '__main__':
    main()
