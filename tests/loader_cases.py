"""Shared by tests/test_loader.py and tests/test_gpu_loader.py: a directory of JPEGs to feed from.

A handful of records of tests/golden/demo_dataset-32.json (the smallest images of each orientation) go into a JSON copy in
the test's ``tmp_path``; their pixels are ``demo_cases.render_image``'s, saved as JPEG with PIL, so every route under
comparison decodes the same files.  Nothing here is committed data."""
import json
import os

import numpy as np

from kgdet_amd import datasets as ds
from tests.golden import demo_cases

SMALL_SCALE = (320, 256)            # an 8 x 10 grid at stride 32: above pos_num = 25


def write_image_dir(root, n=12, no_anno=None, truncate=None):
    """``n`` demo records as ``root/demo.json`` + ``root/image/*.jpg`` -> (ann_file, img_prefix).  ``no_anno``: the record at
    this place keeps only crowd annotations (no ground-truth box survives ``get_ann_info``: the resample path);
    ``truncate``: the JPEG at this place is cut short (a decoder error in the middle of an epoch)."""
    from PIL import Image
    with open(demo_cases.ANN) as f:
        full = json.load(f)
    by_area = sorted(full['images'], key=lambda im: (im['width'] * im['height'], im['id']))
    wide = [im for im in by_area if im['width'] > im['height']][:max(n // 4, 1)]
    tall = [im for im in by_area if im['width'] <= im['height']][:n - len(wide)]
    images = sorted(wide + tall, key=lambda im: im['id'])
    ids = set(im['id'] for im in images)
    anns = [dict(a) for a in full['annotations'] if a['image_id'] in ids]
    if no_anno is not None:
        for a in anns:
            if a['image_id'] == images[no_anno]['id']:
                a['iscrowd'] = 1
    os.makedirs(os.path.join(root, 'image'), exist_ok=True)
    for k, im in enumerate(images):
        mine = [a for a in full['annotations'] if a['image_id'] == im['id']]
        path = os.path.join(root, 'image', im['file_name'])
        Image.fromarray(demo_cases.render_image(im, mine, seed=1000 + k)).save(path, quality=90)
        if truncate == k:
            with open(path, 'rb') as f:
                head = f.read()
            with open(path, 'wb') as f:
                f.write(head[:len(head) // 3])
    ann_file = os.path.join(root, 'demo.json')
    with open(ann_file, 'w') as f:
        json.dump(dict(images=images, annotations=anns, categories=full['categories']), f)
    return ann_file, os.path.join(root, 'image') + os.sep


def dataset_args(ann_file, img_prefix, **kw):
    """the demo config's train pipeline at the small scale"""
    args = dict(ann_file=ann_file, img_prefix=img_prefix, img_scale=SMALL_SCALE, img_norm_cfg=demo_cases.IMG_NORM,
                size_divisor=32, flip_ratio=0.5, with_mask=False, with_crowd=False, with_label=True, with_keypoint=True)
    args.update(kw)
    return args


def train_dataset(ann_file, img_prefix, **kw):
    return ds.DeepFashion2Dataset(**dataset_args(ann_file, img_prefix, **kw))


def test_dataset(ann_file, img_prefix, **kw):
    kw = dict(dict(flip_ratio=0, with_label=False, test_mode=True), **kw)
    return ds.DeepFashion2Dataset(**dataset_args(ann_file, img_prefix, **kw))


test_dataset.__test__ = False        # (a helper, not a test)

EXTRA_AUG = dict(photo_metric_distortion=dict(brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5),
                                              hue_delta=18),
                 expand=dict(mean=demo_cases.IMG_NORM['mean'], to_rgb=demo_cases.IMG_NORM['to_rgb'], ratio_range=(1, 2)),
                 random_crop=dict(min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.3))


def demo_config(ann_file, img_prefix, work_dir, img_scale=SMALL_SCALE, **top):
    """the demo config's values (kgdet_moment_r50_fpn_1x-demo.py) as a plain dict, at the small scale, for one epoch, logging
    every iteration (``img_scale``: ``demo_cases.IMG_SCALE`` for the config's own)"""
    from kgdet_amd import configs
    base = configs.kgdet_r50_fpn()
    common = dict(type='DeepFashion2Dataset', ann_file=ann_file, img_prefix=img_prefix, img_scale=img_scale,
                  img_norm_cfg=dict(demo_cases.IMG_NORM), size_divisor=32, with_keypoint=True, with_mask=False,
                  with_crowd=False, with_label=True)
    cfg = dict(model=_plain(base.model), train_cfg=_plain(base.train_cfg), test_cfg=_plain(base.test_cfg),
               data=dict(imgs_per_gpu=2, workers_per_gpu=2, train=dict(common, flip_ratio=0.5, group_mode=False),
                         val=dict(common, flip_ratio=0), test=dict(common, flip_ratio=0, with_label=False, test_mode=True)),
               optimizer=dict(type='Adam', lr=1e-4), optimizer_config=dict(grad_clip=dict(max_norm=35, norm_type=2)),
               lr_config=dict(policy='step', warmup='linear', warmup_iters=500, warmup_ratio=1.0 / 3, step=[8, 11]),
               checkpoint_config=dict(interval=1), log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')]),
               total_epochs=1, work_dir=work_dir, load_from=None, resume_from=None)
    cfg.update(top)
    return cfg


def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_plain(x) for x in v)
    return v


def write_config_file(path, cfg):
    """``cfg`` as a config file of the reference's kind: one assignment per top-level key"""
    with open(path, 'w') as f:
        for key, value in cfg.items():
            f.write('%s = %r\n' % (key, value))
    return path


def same_value(a, b):
    """deep equality of what the loader yields: tensors and arrays bit for bit, containers element for element"""
    import torch
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape
                and torch.equal(a.cpu(), b.cpu()))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.asarray(a).shape == np.asarray(b).shape and np.asarray(a).dtype == np.asarray(b).dtype and \
            np.array_equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(same_value(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    if hasattr(a, '__dict__') and type(a) is type(b) and not callable(a):
        return same_value(vars(a), vars(b))
    return a == b


def same_rng_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
