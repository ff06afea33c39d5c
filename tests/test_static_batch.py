"""static_batch.StaticBatch on the host: what ``check`` refuses (before anything is copied -- these objects own no buffer at
all) and the table of a mixed batch."""
import pytest
import torch

from kgdet_amd import static_batch as sb

K = 294


def _static(canvas=(800, 1344), cap=8, images=2):
    return sb.StaticBatch(images, canvas, cap, K, 32, 25)        # (device=None: no buffers)


def _batch(counts=(2, 3), hw=(800, 1344), pads=None, key='img_meta'):
    pads = pads or [hw + (3, )] * len(counts)
    return {'img': torch.zeros((len(counts), 3) + tuple(hw)), key: [dict(pad_shape=p) for p in pads],
            'gt_bboxes': [torch.zeros((n, 4)) for n in counts],
            'gt_labels': [torch.zeros((n, ), dtype=torch.int64) for n in counts],
            'gt_keypoints': [torch.zeros((n, K, 3)) for n in counts]}


def test_a_fitting_batch_passes_under_either_meta_key():
    s = _static()
    assert s.img is None and s.table is None
    s.check(_batch())
    s.check(_batch(key='img_metas'))
    s.check(_batch(counts=(8, 1), hw=(704, 1120)))


def _three_images():
    return _batch(counts=(1, 1, 1))


def _no_gt():
    return _batch(counts=(2, 0))


def _too_many():
    return _batch(counts=(9, 1))


def _too_large():
    return _batch(hw=(832, 1344))


def _too_few_points():
    return _batch(pads=[(800, 1344, 3), (128, 160, 3)])          # 4 x 5 = 20 points < pos_num = 25


def _ignore():
    b = _batch()
    b['gt_bboxes_ignore'] = [torch.zeros((0, 4)), torch.zeros((1, 4))]
    return b


def _img_dtype():
    b = _batch()
    b['img'] = b['img'].half()
    return b


def _label_dtype():
    b = _batch()
    b['gt_labels'][1] = b['gt_labels'][1].int()
    return b


def _box_dtype():
    b = _batch()
    b['gt_bboxes'][0] = b['gt_bboxes'][0].double()
    return b


@pytest.mark.parametrize('make, words', [
    (_three_images, 'a batch of 2 images'), (_no_gt, 'No gt or bboxes'), (_too_many, 'the capacity is 8'),
    (_too_large, 'larger than the canvas'), (_too_few_points, 'fewer than pos_num'), (_ignore, 'gt_bboxes_ignore'),
    (_img_dtype, 'float32'), (_label_dtype, 'int64'), (_box_dtype, 'float32')])
def test_check_refuses(make, words):
    s = _static()
    with pytest.raises(ValueError, match=words):
        s.check(make())
    with pytest.raises(ValueError, match=words):       # `load` checks first: a static batch without buffers gets no further
        s.load(make())
    assert s.loads == 0


def test_table_of_a_mixed_batch():
    s = _static()
    table = s.table_of(_batch(counts=(3, 5), pads=[(704, 1120, 3), (800, 1344, 3)]))
    assert table.dtype.name == 'int32' and table.tolist() == [[3, 22, 35, 0], [5, 25, 42, 0]]
    # extents never exceed the canvas's grid; a pad_shape that is no multiple of the stride rounds up
    assert s.table_of(_batch(counts=(1, 1), pads=[(810, 2000, 3), (705, 1121, 3)])).tolist() == [[1, 25, 42, 0], [1, 23, 36, 0]]


def test_constructor_refuses_what_the_kernels_cannot_hold():
    for bad in (dict(cap=0), dict(cap=65), dict(canvas=(800, 1340)), dict(images=17), dict(canvas=(128, 128))):
        with pytest.raises(ValueError):
            _static(**bad)


def test_only_the_kgdet_head_takes_a_table():
    from kgdet_amd import build_detector, configs
    cfg = configs.kgdet_r50_fpn()
    kgdet = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    s = sb.StaticBatch.for_model(kgdet, 2, (800, 1344), 8)
    assert (s.K, s.stride, s.pos_num, s.grid) == (294, 32, 25, (25, 42)) and s.img is None
    cfg = configs.reppoints_kp_r50_fpn(soft_nms=True)
    serial = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    with pytest.raises(NotImplementedError):
        sb.StaticBatch.for_model(serial, 2, (800, 1344), 8)
    b = _batch()
    with pytest.raises(NotImplementedError):          # (refused before anything is computed)
        serial.forward_train(b['img'], b['img_meta'], b['gt_bboxes'], b['gt_labels'], b['gt_keypoints'],
                             gt_table=torch.zeros((2, 4), dtype=torch.int32))
