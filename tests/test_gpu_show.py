"""The routes over ``kgdet_draw_detections``: ``visualize.DeviceDrawer``, ``single_gpu_test(..., show_dir=...)``,
``tools/test.py --show-dir / --out`` and ``RepPointsDetectorKp.show_result``.  The bar is equality with
``visualize.draw_restatement`` on the same image and detections, and results that do not change when pictures are asked for."""
import filecmp
import importlib.util
import io
import os
import pickle
import threading

import numpy as np
import pytest
import torch

from kgdet_amd import visualize as vz
from kgdet_amd.checkpoint import save_checkpoint
from kgdet_amd.runner import DeviceResults, single_gpu_test
from tests import draw_cases as dc
from tests import loader_cases as lc
from tests.golden import demo_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.055                  # the demo detector's scores lie between 0.05 and 0.065: some rows on either side


def _to_dev(t):
    return t.cuda(non_blocking=True)


def _same_result(a, b):
    if len(a) != len(b):
        return False
    if len(a) == 1:
        return all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
    return (all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1])
            and all(np.array_equal(x, y) for x, y in zip(a[2], b[2])))


def _writer_threads():
    return [t for t in threading.enumerate() if t.name.startswith('kgdet-show-writer')]


def test_device_drawer_takes_host_arrays_and_device_tensors():
    sizes = [(33, 65), (70, 100), (1, 1), (16, 64)]
    images = [dc.image(H, W, seed=80 + k) for k, (H, W) in enumerate(sizes)]
    block = np.stack([dc.random_rows(90 + k, 9, 3, H, W, 3) for k, (H, W) in enumerate(sizes)])
    drawer = vz.DeviceDrawer(dc.NAMES3, contour=True, radius=3)
    want = [vz.draw_restatement(img, rows, vz.row_count(rows), dc.NAMES3, contour=True, radius=3) for img, rows in zip(images, block)]
    from_host = drawer(images, block)
    assert all(t.is_cuda and t.dtype == torch.uint8 for t in from_host)
    mixed = [torch.from_numpy(img).cuda() if k % 2 else img for k, img in enumerate(images)]
    from_mixed = drawer(mixed, torch.from_numpy(block).cuda(), to_host=True)
    from_device = drawer([torch.from_numpy(img).cuda() for img in images], torch.from_numpy(block).cuda())
    for w, a, b, c in zip(want, from_host, from_mixed, from_device):
        assert np.array_equal(a.cpu().numpy(), w) and np.array_equal(b, w) and np.array_equal(c.cpu().numpy(), w)
    many = [dc.image(7, 5, seed=k) for k in range(vz.MAX_IMAGES + 3)]        # more than one launch's images
    rows = dc.random_rows(99, 6, 3, 7, 5, 3)
    for got, img in zip(drawer(many, rows[None], to_host=True, blocks=[0] * len(many)), many):
        assert np.array_equal(got, vz.draw_restatement(img, rows, 6, dc.NAMES3, contour=True, radius=3))
    assert drawer([], block) == []
    with pytest.raises(TypeError):
        drawer([images[0].astype(np.float32)], block)
    with pytest.raises(ValueError):
        drawer(images, block[:2])


@pytest.fixture(scope='module')
def demo():
    """the demo detector and the first four demo images; the first run only visits the shapes, the second is the yardstick"""
    cfg, model = demo_cases.demo_detector()
    model = model.cuda()
    data = demo_cases.demo_dataset(test_mode=True)
    data.img_infos = data.img_infos[:4]
    single_gpu_test(model, data, rescale=True, to_device=_to_dev, imgs_per_gpu=4)
    plain = single_gpu_test(model, data, rescale=True, to_device=_to_dev, imgs_per_gpu=4)
    return model, data, plain


def _want(data, i, rows, count):
    return vz.draw_restatement(data.load_image(i), rows, count, data.CLASSES, landmark_ranges=vz.default_ranges(13, 294),
                               score_thr=THR)


def _decoded(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert('RGB'))


def test_show_dir_leaves_the_results_alone_and_writes_the_restatement(demo, tmp_path):
    model, data, plain = demo
    shown = single_gpu_test(model, data, rescale=True, to_device=_to_dev, imgs_per_gpu=4, show_dir=str(tmp_path / 'host'),
                            show_score_thr=THR, show_ext='.png')
    assert len(shown) == len(plain) == 4 and all(_same_result(a, b) for a, b in zip(shown, plain))
    assert sorted(os.listdir(str(tmp_path / 'host'))) == sorted(info['filename'] + '.png' for info in data.img_infos)
    changed = 0
    for i, result in enumerate(plain):
        rows, n = vz.result_rows(result)
        got = _decoded(str(tmp_path / 'host' / (data.img_infos[i]['filename'] + '.png')))
        assert np.array_equal(got, _want(data, i, rows, n)), i
        changed += int((got != data.load_image(i)).any())
    assert changed > 0 and not _writer_threads()
    with pytest.raises(ValueError):
        single_gpu_test(model, data, rescale=False, to_device=_to_dev, show_dir=str(tmp_path / 'never'))
    assert not os.path.exists(str(tmp_path / 'never'))


def test_show_dir_on_the_device_routes(demo, tmp_path):
    model, data, _ = demo
    kw = dict(rescale=True, imgs_per_gpu=4, device_preprocess=True, device_results=True, workers=2)
    single_gpu_test(model, data, **kw)
    plain = single_gpu_test(model, data, **kw)
    shown = single_gpu_test(model, data, show_dir=str(tmp_path / 'dev'), show_score_thr=THR, show_ext='.png', **kw)
    assert isinstance(shown, DeviceResults) and torch.equal(shown.rows, plain.rows)
    block = shown.rows.cpu().numpy()
    for i in range(4):
        got = _decoded(str(tmp_path / 'dev' / (data.img_infos[i]['filename'] + '.png')))
        assert np.array_equal(got, _want(data, i, block[i], vz.row_count(block[i]))), i
    assert not _writer_threads()


def test_a_writer_that_raises_surfaces_and_leaves_no_thread(demo, tmp_path):
    model, data, _ = demo
    os.makedirs(str(tmp_path / 'bad' / (data.img_infos[1]['filename'] + '.png')))      # a directory where a picture should go
    with pytest.raises(OSError):
        single_gpu_test(model, data, rescale=True, to_device=_to_dev, show_dir=str(tmp_path / 'bad'), show_ext='.png', workers=2)
    assert not _writer_threads()
    with pytest.raises(ValueError):
        single_gpu_test(model, data, rescale=True, to_device=_to_dev, show_dir=str(tmp_path / 'ext'), show_ext='.gif')


def test_model_show_result_equals_the_restatement_on_the_denormalised_crop(demo):
    model, data, _ = demo
    sample = data[0]
    collated = dict(img=[sample['img'][0][None]], img_meta=[[sample['img_meta'][0]]])
    with torch.no_grad():
        result = model([collated['img'][0].cuda()], collated['img_meta'], return_loss=False, rescale=False)
    model.CLASSES = data.CLASSES
    try:
        out = model.show_result(collated, result, demo_cases.IMG_NORM, score_thr=0.0)
        assert out[0].tobytes() == model.show_result(collated, result, demo_cases.IMG_NORM, dataset=list(data.CLASSES), score_thr=0.0)[0].tobytes()
        with pytest.raises(TypeError):
            model.show_result(collated, result, demo_cases.IMG_NORM, dataset='coco')
    finally:
        del model.CLASSES
    h, w = sample['img_meta'][0]['img_shape'][:2]
    crop = np.ascontiguousarray(vz.denormalize(sample['img'][0].numpy(), **demo_cases.IMG_NORM)[:h, :w])
    rows, n = vz.result_rows(result)
    want = vz.draw_restatement(crop, rows, n, data.CLASSES, landmark_ranges=vz.default_ranges(13, 294), score_thr=0.0)
    assert len(out) == 1 and np.array_equal(out[0], want) and n > 0 and (want != crop).any()


def _tool(name):
    spec = importlib.util.spec_from_file_location('kgdet_tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_test_tool_with_show_dir_and_out(tmp_path):
    """(at the config's own scale, where the detector repeats itself bit for bit -- tests/test_gpu_loader.py; the first run
    only visits the shapes)"""
    from PIL import Image
    from kgdet_amd import Config
    from kgdet_amd.apis import init_detector
    from kgdet_amd.datasets import build_dataset
    ann, prefix = lc.write_image_dir(str(tmp_path / 'set'), n=4)
    config = lc.write_config_file(str(tmp_path / 'demo.py'), lc.demo_config(ann, prefix, str(tmp_path / 'work'),
                                                                            img_scale=demo_cases.IMG_SCALE))
    ckpt = str(tmp_path / 'demo.pth')
    save_checkpoint(demo_cases.demo_detector()[1], ckpt)
    tool = _tool('test')
    tool.main([config, ckpt, '--json_out', str(tmp_path / 'warm')])
    tool.main([config, ckpt, '--json_out', str(tmp_path / 'plain')])
    tool.main([config, ckpt, '--json_out', str(tmp_path / 'shown'), '--show-dir', str(tmp_path / 'pictures'), '--show-score-thr',
               str(THR), '--out', str(tmp_path / 'results.pkl')])
    for kind in ('bbox', 'keypoints'):
        assert os.path.getsize(str(tmp_path / ('plain.%s.json' % kind))) > 2
        assert filecmp.cmp(str(tmp_path / ('shown.%s.json' % kind)), str(tmp_path / ('plain.%s.json' % kind)), shallow=False), kind
    cfg = Config.fromfile(config)
    cfg.data.test.test_mode = True
    data = build_dataset(cfg.data.test)
    plain = single_gpu_test(init_detector(cfg, ckpt, device='cuda:0'), data, rescale=True, to_device=_to_dev, workers=2)
    with open(str(tmp_path / 'results.pkl'), 'rb') as f:
        pickled = pickle.load(f)
    assert len(pickled) == len(plain) == 4 and all(_same_result(a, b) for a, b in zip(pickled, plain))
    names = sorted(os.path.basename(info['filename']) + '.jpg' for info in data.img_infos)
    assert sorted(os.listdir(str(tmp_path / 'pictures'))) == names
    for i, result in enumerate(plain):
        rows, n = vz.result_rows(result)
        buf = io.BytesIO()
        Image.fromarray(_want(data, i, rows, n)).save(buf, format='JPEG', quality=90)
        with open(str(tmp_path / 'pictures' / (os.path.basename(data.img_infos[i]['filename']) + '.jpg')), 'rb') as f:
            assert f.read() == buf.getvalue(), i
    with pytest.raises(SystemExit):
        tool.main([config, ckpt, '--out', str(tmp_path / 'results.txt')])
