"""Entry points that run a config end to end, for one process and one GPU: ``mmdet/apis/train.py`` (``train_detector``,
``set_random_seed``) and ``mmdet/apis/inference.py`` (``init_detector``, ``inference_detector``, and ``show_result``, which
``visualize`` draws -- landmarks included -- on the GPU or, without one, with its numpy restatement).
``tools/train.py`` and ``tools/test.py`` are thin command lines over these and ``runner.single_gpu_test``."""
import json
import os
import random
import time

import numpy as np
import torch

from . import datasets as ds
from .checkpoint import load_checkpoint
from .loader import build_dataloader
from .registry import Config, ConfigDict, build_detector
from .runner import Runner, build_optimizer, single_gpu_test
from .visualize import show_result  # noqa: F401  (mmdet.apis.show_result)


def set_random_seed(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def _get(cfg, key, default=None):
    value = cfg.get(key, default) if hasattr(cfg, 'get') else getattr(cfg, key, default)
    return default if value is None else value


def train_detector(model, dataset, cfg, validate=False, logger=None):
    """``mmdet.apis.train_detector`` (the ``_non_dist_train`` flow) -> the ``Runner`` after ``cfg.total_epochs``.

    The loader is ``build_dataloader(dataset, cfg.data.imgs_per_gpu, cfg.data.workers_per_gpu, device=<the model's GPU>)``; the
    optional config key ``loader = dict(device_preprocess=..., device_decode=..., prefetch=...)`` picks the feed's route (absent: host pixels,
    uploaded from page-locked memory).  The runner takes ``cfg.lr_config``, ``cfg.optimizer_config``, ``cfg.checkpoint_config``,
    ``cfg.log_config.interval`` and ``cfg.work_dir``; ``cfg.resume_from`` / ``cfg.load_from`` are honoured in that order.
    ``validate=True``: ``cfg.data.val`` (built in test mode) is evaluated after every ``cfg.evaluation.interval``-th epoch
    (default 1) with the loader's route and worker count.  Every log record is appended as one JSON line to
    ``work_dir/<timestamp>.log.json`` with mmcv's ``mode`` field ('train' / 'val').  A model on the CPU is moved to the current
    GPU first.  Nothing here seeds an RNG (``set_random_seed``) or fetches weights."""
    logger = logger or print
    if isinstance(cfg, dict) and not isinstance(cfg, ConfigDict):
        cfg = ConfigDict(cfg)
    if not any(p.is_cuda for p in model.parameters()):
        model = model.cuda()
    device = next(model.parameters()).device
    opts = dict(_get(cfg, 'loader', {}))
    device_preprocess = bool(opts.get('device_preprocess', False))
    device_decode = opts.get('device_decode', False)           # False, True or 'camera' (jpeg.decode_switch)
    loader = build_dataloader(dataset, cfg.data.imgs_per_gpu, cfg.data.workers_per_gpu, _get(cfg, 'gpus', 1), dist=False,
                              device=device, device_preprocess=device_preprocess, prefetch=opts.get('prefetch', 2),
                              device_decode=device_decode)
    optimizer = build_optimizer(model, cfg.optimizer)
    work_dir = _get(cfg, 'work_dir')
    log_path = None
    if work_dir is not None:
        os.makedirs(work_dir, exist_ok=True)
        log_path = os.path.join(work_dir, time.strftime('%Y%m%d_%H%M%S') + '.log.json')

    def on_record(mode, rec):
        if log_path is not None:
            line = dict(mode=mode)
            line.update(rec)
            with open(log_path, 'a') as f:
                f.write(json.dumps(line) + '\n')

    eval_config = None
    if validate:
        val = ds.build_dataset(cfg.data.val, dict(test_mode=True))
        eval_config = dict(dataset=val, interval=dict(_get(cfg, 'evaluation', {})).get('interval', 1),
                           imgs_per_gpu=cfg.data.imgs_per_gpu, device_preprocess=device_preprocess, device_decode=device_decode,
                           workers=min(cfg.data.workers_per_gpu, 16), to_device=lambda t: t.to(device, non_blocking=True))
    runner = Runner(model, optimizer, work_dir=work_dir, lr_config=_get(cfg, 'lr_config'),
                    optimizer_config=_get(cfg, 'optimizer_config'), checkpoint_config=_get(cfg, 'checkpoint_config'),
                    log_interval=dict(_get(cfg, 'log_config', {})).get('interval', 50), logger=logger,
                    eval_config=eval_config, on_record=on_record)
    if _get(cfg, 'resume_from'):
        runner.resume(cfg.resume_from, map_location=str(device))
    elif _get(cfg, 'load_from'):
        load_checkpoint(model, cfg.load_from, map_location='cpu')
    try:
        runner.run(loader, cfg.total_epochs, to_device=None, set_epoch=loader.set_epoch)
    finally:
        loader.close()
    return runner


def init_detector(config, checkpoint=None, device='cuda:0'):
    """``mmdet.apis.init_detector``: the detector of ``config`` (a path or a ``Config``) with ``checkpoint``'s weights, on
    ``device``, in ``eval()``; the config is kept as ``model.cfg`` for ``inference_detector``.  ``pretrained`` is dropped: nothing
    is fetched."""
    if isinstance(config, str):
        config = Config.fromfile(config)
    elif not isinstance(config, Config):
        raise TypeError('config must be a filename or Config object, but got {}'.format(type(config)))
    config.model.pretrained = None
    model = build_detector(config.model, test_cfg=config.test_cfg)
    model.CLASSES = ds.DeepFashion2Dataset.CLASSES
    if checkpoint is not None:
        ckpt = load_checkpoint(model, checkpoint, map_location='cpu')
        if isinstance(ckpt, dict) and 'CLASSES' in ckpt.get('meta', {}):
            model.CLASSES = ckpt['meta']['CLASSES']
    model.cfg = config
    model.to(device)
    model.eval()
    return model


class ImageList(ds.DeepFashion2Dataset):
    """images without annotations behind the dataset's test-time interface (``prepare_test_img`` / ``prepare_test_raw``): file
    paths or decoded uint8 H x W x 3 RGB arrays, with the test pipeline's settings of a ``cfg.data.test`` dict"""

    def __init__(self, images, img_scale, img_norm_cfg, size_divisor=None, flip_ratio=0, resize_keep_ratio=True, **unused):
        ds.landmark_fields(self)
        self.images = list(images)
        self.img_infos = [self._info(img) for img in self.images]         # (a path: the size from the file's header)
        self.img_scales = img_scale if isinstance(img_scale, list) else [img_scale]
        self.img_norm_cfg, self.size_divisor, self.flip_ratio = img_norm_cfg, size_divisor, flip_ratio
        self.resize_keep_ratio, self.test_mode, self.extra_aug = resize_keep_ratio, True, None
        self.img_transform = ds.ImageTransform(size_divisor=size_divisor, **img_norm_cfg)

    @staticmethod
    def _info(img):
        if isinstance(img, str):
            from PIL import Image
            with Image.open(img) as im:
                return dict(height=im.size[1], width=im.size[0], filename=img)
        if not (isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3):
            raise TypeError('an image is a path or a decoded uint8 H x W x 3 RGB array')
        return dict(height=img.shape[0], width=img.shape[1], filename=None)

    def load_image(self, idx):
        img = self.images[idx]
        if isinstance(img, str):
            from PIL import Image
            with Image.open(img) as im:
                img = np.array(im.convert('RGB'))
        return img


def inference_detector(model, img_or_paths, device_preprocess=False, workers=0):
    """``mmdet.apis.inference_detector``: one image (a path or a decoded uint8 RGB array) -> its result, a list of them -> the
    list of results -- what ``single_gpu_test`` returns per image, through the same loop: the test transform of
    ``model.cfg.data.test`` on the host, or ``DeviceImageTransform`` with ``device_preprocess=True``."""
    single = isinstance(img_or_paths, (str, np.ndarray))
    images = ImageList([img_or_paths] if single else img_or_paths, **dict(model.cfg.data.test))
    device = next(model.parameters()).device
    results = single_gpu_test(model, images, rescale=True, to_device=lambda t: t.to(device),
                              device_preprocess=device_preprocess, workers=workers)
    return results[0] if single else results
