"""The routes over ``kgdet_jpeg_encode`` / ``kgdet_jpeg_write``: ``jpeg.DeviceJpegEncoder``, ``jpeg.encode_jpeg``,
``single_gpu_test(..., show_dir=..., show_encoder='device')`` and ``tools/test.py --show-encoder device``, on the demo detector
and the four demo images tests/test_gpu_show.py uses.  The bar is equality of the files with
``jpeg.jpeg_restatement(visualize.draw_restatement(...))``, results that do not change, and a default route that writes what it
wrote before."""
import importlib.util
import io
import os
import threading

import numpy as np
import pytest
import torch

from kgdet_amd import jpeg
from kgdet_amd import visualize as vz
from kgdet_amd.checkpoint import save_checkpoint
from kgdet_amd.runner import single_gpu_test
from tests import jpeg_refs as jr
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


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def test_device_encoder_takes_views_of_one_buffer_and_separate_tensors(tmp_path):
    names = ['noise-17x9', 'ramp-24x40', 'noise-80x96', 'grey-1x1']
    want = [jr.restated(name, 90)['bytes'] for name in names]
    tensors = [torch.from_numpy(np.array(jr.image(name))).cuda() for name in names]
    encoder = jpeg.DeviceJpegEncoder()
    assert encoder(tensors) == want and encoder.downloaded >= sum(len(w) for w in want)
    flat = torch.zeros(sum(t.numel() + 7 for t in tensors), dtype=torch.uint8, device='cuda')
    views, at = [], 5
    for t in tensors:
        views.append(flat[at:at + t.numel()].view(t.shape))
        views[-1].copy_(t)
        at += t.numel() + 7
    assert encoder(views) == want and encoder(views[::-1]) == want[::-1]
    assert encoder([tensors[2][:, :9]]) == [jpeg.jpeg_restatement(np.ascontiguousarray(jr.image(names[2])[:, :9]))]     # not contiguous
    many = [tensors[k % 2] for k in range(jpeg.MAX_IMAGES + 3)]                   # more than one call's images
    assert encoder(many) == [want[k % 2] for k in range(len(many))]
    assert encoder([]) == []
    assert jpeg.DeviceJpegEncoder(50)([tensors[0]]) == [jr.restated(names[0], 50)['bytes'] if (names[0], 50) in jr.RUNS
                                                         else jpeg.jpeg_restatement(jr.image(names[0]), 50)]
    assert jpeg.encode_jpeg(jr.image(names[1])) == want[1] and jpeg.encode_jpeg(tensors[1], quality=90) == want[1]
    for bad in (jr.image(names[0]), tensors[0].float(), tensors[0][..., :2]):
        with pytest.raises(TypeError):
            encoder([bad])
    with pytest.raises(ValueError):
        jpeg.DeviceJpegEncoder(0)
    writer = vz.PictureWriter(str(tmp_path / 'w'), workers=2)
    writer.put_bytes(want[0], 'a')
    writer.put(np.ascontiguousarray(jr.image(names[0])), 'b')
    writer.close()
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(jr.image(names[0])).save(buf, format='JPEG', quality=90)
    assert _read(str(tmp_path / 'w' / 'a.jpg')) == want[0] and _read(str(tmp_path / 'w' / 'b.jpg')) == buf.getvalue()
    assert not _writer_threads()


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


def _drawn(data, i, result):
    rows, n = vz.result_rows(result)
    return vz.draw_restatement(data.load_image(i), rows, n, data.CLASSES, landmark_ranges=vz.default_ranges(13, 294), score_thr=THR)


def test_device_encoder_route_leaves_the_results_alone_and_writes_the_restatement(demo, tmp_path):
    from PIL import Image
    model, data, plain = demo
    with pytest.raises(ValueError):
        single_gpu_test(model, data, rescale=True, to_device=_to_dev, show_dir=str(tmp_path / 'never'), show_ext='.png',
                        show_encoder='device')
    with pytest.raises(ValueError):
        single_gpu_test(model, data, rescale=True, to_device=_to_dev, show_dir=str(tmp_path / 'never'), show_encoder='gpu')
    assert not os.path.exists(str(tmp_path / 'never'))
    shown = single_gpu_test(model, data, rescale=True, to_device=_to_dev, imgs_per_gpu=4, show_dir=str(tmp_path / 'dev'),
                            show_score_thr=THR, show_encoder='device', workers=2)
    assert len(shown) == len(plain) == 4 and all(_same_result(a, b) for a, b in zip(shown, plain))
    assert sorted(os.listdir(str(tmp_path / 'dev'))) == sorted(info['filename'] + '.jpg' for info in data.img_infos)
    changed = 0
    for i, result in enumerate(plain):
        drawn = _drawn(data, i, result)
        path = str(tmp_path / 'dev' / (data.img_infos[i]['filename'] + '.jpg'))
        assert _read(path) == jpeg.jpeg_restatement(drawn), i
        with Image.open(path) as im:
            assert im.format == 'JPEG' and im.size == (drawn.shape[1], drawn.shape[0])
            changed += int(np.abs(np.array(im.convert('RGB')).astype(int) - data.load_image(i)).max() > 64)
    assert changed > 0 and not _writer_threads()


def test_the_default_route_writes_what_the_host_writer_makes_of_the_drawn_array(demo, tmp_path):
    model, data, plain = demo
    shown = single_gpu_test(model, data, rescale=True, to_device=_to_dev, imgs_per_gpu=4, show_dir=str(tmp_path / 'host'),
                            show_score_thr=THR)
    explicit = single_gpu_test(model, data, rescale=True, to_device=_to_dev, imgs_per_gpu=4, show_dir=str(tmp_path / 'host2'),
                               show_score_thr=THR, show_encoder='host')
    assert all(_same_result(a, b) for a, b in zip(shown, plain)) and all(_same_result(a, b) for a, b in zip(explicit, plain))
    writer = vz.PictureWriter(str(tmp_path / 'want'))
    for i, result in enumerate(plain):
        writer.put(_drawn(data, i, result), data.img_infos[i]['filename'])
    writer.close()
    for info in data.img_infos:
        want = _read(str(tmp_path / 'want' / (info['filename'] + '.jpg')))
        assert _read(str(tmp_path / 'host' / (info['filename'] + '.jpg'))) == want
        assert _read(str(tmp_path / 'host2' / (info['filename'] + '.jpg'))) == want
    assert not _writer_threads()


def test_device_results_route_with_the_device_encoder(demo, tmp_path):
    model, data, _ = demo
    kw = dict(rescale=True, imgs_per_gpu=4, device_preprocess=True, device_results=True, workers=2)
    single_gpu_test(model, data, **kw)
    plain = single_gpu_test(model, data, **kw)
    shown = single_gpu_test(model, data, show_dir=str(tmp_path / 'dev'), show_score_thr=THR, show_encoder='device', **kw)
    assert torch.equal(shown.rows, plain.rows)
    block = shown.rows.cpu().numpy()
    for i in range(4):
        drawn = vz.draw_restatement(data.load_image(i), block[i], vz.row_count(block[i]), data.CLASSES,
                                    landmark_ranges=vz.default_ranges(13, 294), score_thr=THR)
        assert _read(str(tmp_path / 'dev' / (data.img_infos[i]['filename'] + '.jpg'))) == jpeg.jpeg_restatement(drawn), i


def test_test_tool_with_the_device_encoder(tmp_path):
    from PIL import Image
    spec = importlib.util.spec_from_file_location('kgdet_tool_test_jpeg', os.path.join(ROOT, 'tools', 'test.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ann, prefix = lc.write_image_dir(str(tmp_path / 'set'), n=2)
    config = lc.write_config_file(str(tmp_path / 'demo.py'), lc.demo_config(ann, prefix, str(tmp_path / 'work'),
                                                                            img_scale=demo_cases.IMG_SCALE))
    ckpt = str(tmp_path / 'demo.pth')
    save_checkpoint(demo_cases.demo_detector()[1], ckpt)
    tool.main([config, ckpt, '--show-dir', str(tmp_path / 'pictures'), '--show-encoder', 'device', '--show-score-thr', str(THR)])
    files = sorted(os.listdir(str(tmp_path / 'pictures')))
    assert len(files) == 2 and all(f.endswith('.jpg') for f in files)
    for f in files:
        data = _read(str(tmp_path / 'pictures' / f))
        parsed = jr.parse(data)
        with Image.open(io.BytesIO(data)) as im:
            im.load()
            assert im.format == 'JPEG' and im.mode == 'RGB' and im.size == (parsed['sof'][2], parsed['sof'][1])
    with pytest.raises(SystemExit):
        tool.parse_args([config, ckpt, '--show-dir', 'x', '--show-encoder', 'png'])
