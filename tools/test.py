"""Test a detector from a config file and a checkpoint (the reference's ``tools/test.py``), one process on one GPU.

    python tools/test.py CONFIG CHECKPOINT [--json_out P] [--eval bbox keypoints] [--workers N] [--imgs-per-gpu N]
                                           [--device-preprocess [--device-decode [--device-decode-files camera]]] [--device-results] [--out FILE.pkl]
                                           [--show-dir DIR] [--show-score-thr T] [--show-encoder {host,device}]
                                           [--grouped-bf16 {0,1,force}]

``cfg.data.test`` goes through ``runner.single_gpu_test``: ``--workers`` threads decode and prepare the upcoming images
(default ``cfg.data.workers_per_gpu``), ``--imgs-per-gpu`` images of one shape share a forward pass, ``--device-preprocess``
runs the input transform on the GPU, ``--device-results`` keeps the detections in device memory until they are evaluated.
``--json_out P`` writes ``P.bbox.json`` / ``P.keypoints.json`` through ``evaluation.results2json`` -- with ``--device-results``
from the rows in device memory (``evaluation_device.results2json_any``: the same bytes, formatted by kernels) -- and evaluates
those files with ``coco_eval``; without it ``--eval`` evaluates the results where they lie (``evaluation_device.evaluate_results``).
``--out FILE.pkl`` is the reference's pickle of the result list (with ``--device-results``: of ``to_host()``).  ``--show-dir DIR``
(the reference's ``--show``, into files): every image with its detections above ``--show-score-thr`` and their landmarks, drawn
on the GPU a group at a time (``kgdet_draw_detections``) and encoded to ``DIR/<image file name>.jpg`` by the ``--workers``
threads; with ``--show-encoder device`` the pictures are encoded on the GPU as well (``kgdet_jpeg_encode``: baseline JPEG at
quality 90, other bytes than PIL's) and the threads only write the files.  ``--grouped-bf16`` sets
``kgdet_amd.grouped_conv.BF16``: the grouped conv2 of a ResNeXt backbone on the bf16 channels-last HIP kernel (``1``: the classes
measured faster than torch's route, ``force``: all; default: ``KGDET_GROUPED_CONV_BF16``, else off).  A ``--launcher`` other than ``none`` is refused:
the multi-rank launch is not part of this tool."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Test a detector')
    parser.add_argument('config', help='test config file path')
    parser.add_argument('checkpoint', help='checkpoint file')
    parser.add_argument('--json_out', help='output result file name without extension')
    parser.add_argument('--eval', nargs='+', choices=['bbox', 'keypoints'], help='eval types')
    parser.add_argument('--workers', type=int, default=None, help='threads that prepare upcoming images')
    parser.add_argument('--imgs-per-gpu', type=int, default=1)
    parser.add_argument('--device-preprocess', action='store_true')
    parser.add_argument('--device-decode', action='store_true',
                        help='decode the JPEG files on the GPU (needs --device-preprocess)')
    parser.add_argument('--device-decode-files', choices=('baseline', 'camera'), default='baseline',
                        help='with --device-decode: which files the GPU decodes; camera adds 4:2:2 files and files with '
                             'restart intervals, which baseline hands to PIL with a warning')
    parser.add_argument('--device-results', action='store_true')
    parser.add_argument('--out', help='output result file (a pickle of the result list)')
    parser.add_argument('--show-dir', help='directory the drawn images are written to')
    parser.add_argument('--show-score-thr', type=float, default=0.3, help='score threshold of the drawn detections')
    parser.add_argument('--show-encoder', choices=['host', 'device'], default='host',
                        help='where the drawn images become JPEG files: PIL in the writer threads, or kernels on the GPU')
    parser.add_argument('--grouped-bf16', choices=['0', '1', 'force'], default=None,
                        help='grouped 3x3 convolutions of a ResNeXt at bf16 inference on the HIP kernel (default: off)')
    parser.add_argument('--launcher', default='none', help='job launcher (only "none")')
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.launcher != 'none':
        raise SystemExit('--launcher %s: this tool runs one process on one GPU (the multi-rank launch is a separate tool)'
                         % args.launcher)
    if not (args.json_out or args.eval or args.out or args.show_dir):
        raise SystemExit('nothing to do: give --json_out, --eval, --out and / or --show-dir')
    if args.device_decode and not args.device_preprocess:
        raise SystemExit('--device-decode needs --device-preprocess')
    if args.out is not None and not args.out.endswith(('.pkl', '.pickle')):
        raise SystemExit('The output file must be a pkl file.')
    import torch
    from kgdet_amd import Config, evaluation, evaluation_device
    from kgdet_amd.apis import init_detector
    from kgdet_amd.datasets import build_dataset
    from kgdet_amd.runner import single_gpu_test
    if not torch.cuda.is_available():
        raise SystemExit('tools/test.py needs a GPU')
    if args.grouped_bf16 is not None:
        from kgdet_amd import grouped_conv
        grouped_conv.BF16 = grouped_conv.parse_bf16(args.grouped_bf16)
    cfg = Config.fromfile(args.config)
    cfg.data.test.test_mode = True
    dataset = build_dataset(cfg.data.test)
    model = init_detector(cfg, args.checkpoint, device='cuda:0')
    workers = cfg.data.get('workers_per_gpu', 0) if args.workers is None else args.workers
    results = single_gpu_test(model, dataset, rescale=True, to_device=lambda t: t.cuda(non_blocking=True),
                              imgs_per_gpu=args.imgs_per_gpu, device_preprocess=args.device_preprocess,
                              device_results=args.device_results, workers=min(workers, 16), show_dir=args.show_dir,
                              show_score_thr=args.show_score_thr, show_encoder=args.show_encoder,
                              device_decode='camera' if args.device_decode and args.device_decode_files == 'camera' else args.device_decode)
    if args.out:
        import pickle
        print('writing results to {}'.format(args.out))
        with open(args.out, 'wb') as f:
            pickle.dump(results.to_host() if args.device_results else results, f)
    stats = None
    if args.json_out:
        out = args.json_out[:-5] if args.json_out.endswith('.json') else args.json_out
        print('writing results to {}'.format(out))
        files = evaluation_device.results2json_any(dataset, results, out)
        if args.eval:
            print('Starting evaluate {}'.format(' and '.join(args.eval)))
            stats = evaluation.coco_eval(files, args.eval, dataset.coco, device='cuda:0')
    elif args.eval:
        print('Starting evaluate {}'.format(' and '.join(args.eval)))
        stats = evaluation_device.evaluate_results(dataset, results, args.eval, device='cuda:0', verbose=True)
    return stats


if __name__ == '__main__':
    main()
