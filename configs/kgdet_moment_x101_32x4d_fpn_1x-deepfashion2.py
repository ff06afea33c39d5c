"""KGDet (moment transform, FPN level 32) on a ResNeXt-101 32x4d backbone, DeepFashion2 train / validation, schedule 1x.

The model, train_cfg and test_cfg are ``kgdet_amd.configs.kgdet_x101_fpn()``: the r50 model with the backbone dict swapped and
``pretrained`` naming the published ``resnext101_32x4d`` weights.

    python tools/train.py configs/kgdet_moment_x101_32x4d_fpn_1x-deepfashion2.py
    python tools/test.py configs/kgdet_moment_x101_32x4d_fpn_1x-deepfashion2.py <checkpoint>
"""
from kgdet_amd import configs as _configs

_base = _configs.kgdet_x101_fpn(groups=32, base_width=4, depth=101)
model = _base.model
train_cfg = _base.train_cfg
test_cfg = _base.test_cfg

dataset_type = 'DeepFashion2Dataset'
data_root = 'data/deepfashion2/'
img_norm_cfg = dict(mean=[154.992, 146.197, 140.744], std=[62.757, 64.507, 62.076], to_rgb=True)
_common = dict(type=dataset_type, img_scale=(1333, 800), img_norm_cfg=img_norm_cfg, size_divisor=32, with_keypoint=True,
               with_mask=False, with_crowd=False, with_label=True)
_train = dict(_common, ann_file=data_root + 'train/train-coco_style.json', img_prefix=data_root + 'train/image/')
_val = dict(_common, ann_file=data_root + 'validation/val-coco_style.json', img_prefix=data_root + 'validation/image/')
data = dict(imgs_per_gpu=2, workers_per_gpu=2,
            train=dict(_train, flip_ratio=0.5, group_mode=False),
            val=dict(_val, flip_ratio=0),
            test=dict(_val, flip_ratio=0, with_label=False, test_mode=True))

optimizer = dict(type='SGD', lr=5e-3, momentum=0.9, weight_decay=1e-4)
optimizer_config = dict(grad_clip=dict(max_norm=35, norm_type=2))
lr_config = dict(policy='step', warmup='linear', warmup_iters=500, warmup_ratio=1.0 / 3, step=[8, 11])
checkpoint_config = dict(interval=1)
log_config = dict(interval=100, hooks=[dict(type='TextLoggerHook')])
total_epochs = 12
log_level = 'INFO'
work_dir = './work_dirs/kgdet_moment_x101_32x4d_fpn_1x-deepfashion2'
load_from = None
resume_from = None
workflow = [('train', 1)]
