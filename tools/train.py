"""Train a detector from a config file (the reference's ``tools/train.py``), one process on one GPU.

    python tools/train.py CONFIG [--work_dir D] [--resume_from P] [--load_from P] [--validate] [--seed N]
                                 [--device-preprocess [--device-decode [--device-decode-files camera]]]

CONFIG is one of the reference's config files, unchanged.  ``--device-preprocess`` feeds the raw pixels to the GPU's input
transform (``loader = dict(device_preprocess=True)``); without it the host pixels go up from page-locked memory.  Checkpoints
and ``<timestamp>.log.json`` land in the work directory.  ``pretrained='modelzoo://...'`` is ignored: nothing is fetched; start
from weights with ``--load_from``.  A ``--launcher`` other than ``none`` is refused: the multi-rank launch is not part of this
tool."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Train a detector')
    parser.add_argument('config', help='train config file path')
    parser.add_argument('--work_dir', help='the dir to save logs and models')
    parser.add_argument('--resume_from', help='the checkpoint file to resume from')
    parser.add_argument('--load_from', help='the checkpoint file to take the weights from')
    parser.add_argument('--validate', action='store_true', help='evaluate cfg.data.val after every epoch')
    parser.add_argument('--seed', type=int, default=None, help='random seed')
    parser.add_argument('--device-preprocess', action='store_true', help='input transform on the GPU from the raw pixels')
    parser.add_argument('--device-decode', action='store_true',
                        help='decode the JPEG files on the GPU too (needs --device-preprocess)')
    parser.add_argument('--device-decode-files', choices=('baseline', 'camera'), default='baseline',
                        help='with --device-decode: which files the GPU decodes; camera adds 4:2:2 files and files with '
                             'restart intervals, which baseline hands to PIL with a warning')
    parser.add_argument('--launcher', default='none', help='job launcher (only "none")')
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.launcher != 'none':
        raise SystemExit('--launcher %s: this tool runs one process on one GPU (the multi-rank launch is a separate tool)'
                         % args.launcher)
    import torch
    from kgdet_amd import Config, build_detector
    from kgdet_amd.apis import set_random_seed, train_detector
    from kgdet_amd.datasets import build_dataset
    if not torch.cuda.is_available():
        raise SystemExit('tools/train.py needs a GPU')
    cfg = Config.fromfile(args.config)
    if args.work_dir is not None:
        cfg.work_dir = args.work_dir
    if args.resume_from is not None:
        cfg.resume_from = args.resume_from
    if args.load_from is not None:
        cfg.load_from = args.load_from
    if args.device_decode and not args.device_preprocess:
        raise SystemExit('--device-decode needs --device-preprocess')
    if args.device_preprocess:
        cfg.loader = dict(cfg.get('loader') or {}, device_preprocess=True)
    if args.device_decode:
        cfg.loader = dict(cfg.get('loader') or {}, device_decode='camera' if args.device_decode_files == 'camera' else True)
    cfg.gpus = 1
    if args.seed is not None:
        print('Set random seed to {}'.format(args.seed))
        set_random_seed(args.seed)
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)       # (initialises its weights)
    dataset = build_dataset(cfg.data.train)
    model.CLASSES = dataset.CLASSES
    train_detector(model.cuda(), dataset, cfg, validate=args.validate)


if __name__ == '__main__':
    main()
