"""The ``device_decode`` routes on the GPU: ``build_dataloader(..., device_preprocess=True, device_decode=True)`` and
``single_gpu_test(..., device_decode=True)`` against the same calls with ``device_decode=False`` -- bit for bit, since the
decoder's pictures are PIL's --, files the decoder does not take or refuses, and a truncated file's error.  JPEGs are written
into tmp_path (tests/loader_cases.py's rendered records)."""
import os
import warnings

import numpy as np
import pytest
import torch

from kgdet_amd import datasets as ds
from kgdet_amd import jpeg
from kgdet_amd import loader as ld
from kgdet_amd import runner as rn
from tests import jpeg_decode_refs as dr
from tests import loader_cases as lc
from tests.golden import demo_cases

pytestmark = pytest.mark.gpu
GT_KEYS = ('gt_bboxes', 'gt_labels', 'gt_keypoints')


@pytest.fixture(scope='module')
def feed_dir(tmp_path_factory):
    return lc.write_image_dir(str(tmp_path_factory.mktemp('feed')), n=12, no_anno=3)


@pytest.fixture(scope='module')
def small_dir(tmp_path_factory):
    return lc.write_image_dir(str(tmp_path_factory.mktemp('small')), n=8)


@pytest.fixture(scope='module')
def detector():
    cfg, model = demo_cases.demo_detector()
    return model.cuda().eval()


def epoch(data, seed, workers, **kw):
    """every batch of one epoch, kept alive, and numpy's RNG state behind it"""
    np.random.seed(seed)
    kept = list(ld.build_dataloader(data, 2, workers, device='cuda', device_preprocess=True, prefetch=3, **kw))
    return kept, np.random.get_state()


def assert_same_batches(got, want):
    assert len(got) == len(want) >= 4
    for a, b in zip(got, want):
        assert a['img'].is_cuda and a['img'].dtype == torch.float32 and torch.equal(a['img'], b['img'])
        assert lc.same_value(a['img_meta'], b['img_meta'])
        for key in GT_KEYS:
            assert len(a[key]) == len(b[key]) and all(x.is_cuda and torch.equal(x, y) for x, y in zip(a[key], b[key]))


@pytest.mark.parametrize('workers', [0, 4])
def test_the_loader_yields_the_same_batches_with_the_files_decoded_on_the_gpu(feed_dir, workers):
    data = lc.train_dataset(*feed_dir, img_scale=[(320, 256), (256, 192)], multiscale_mode='range', extra_aug=lc.EXTRA_AUG)
    want, state = epoch(data, 11, workers)
    with warnings.catch_warnings():
        warnings.simplefilter('error')                      # every file is one the decoder takes: nothing falls back
        got, state_decode = epoch(data, 11, workers, device_decode=True)
    assert lc.same_rng_state(state_decode, state)
    assert_same_batches(got, want)
    plain = lc.train_dataset(*feed_dir)                     # and without extra_aug
    assert_same_batches(epoch(plain, 5, workers, device_decode=True)[0], epoch(plain, 5, workers)[0])
    torch.cuda.synchronize()


def test_device_decode_needs_the_device_route(feed_dir):
    data = lc.train_dataset(*feed_dir)
    with pytest.raises(ValueError, match='device_preprocess'):
        ld.build_dataloader(data, 2, 0, device='cuda', device_decode=True)
    with pytest.raises(ValueError, match='device_preprocess'):
        ld.build_dataloader(data, 2, 0, device_preprocess=True, device_decode=True)
    with pytest.raises(ValueError, match='device_preprocess'):
        rn.single_gpu_test(None, lc.test_dataset(*feed_dir), device_decode=True)


def test_load_image_file_carries_the_header_shape(feed_dir):
    data = lc.train_dataset(*feed_dir)
    enc = data.load_image_file(0)
    img = data.load_image(0)
    assert isinstance(enc, ds.EncodedImage) and enc.shape == img.shape and enc.reason is None and enc.pixels is None
    assert np.array_equal(jpeg.decode_restatement(enc.data), img)
    np.random.seed(3)
    a = data.prepare_train_raw(0, img=enc)
    np.random.seed(3)
    b = data.prepare_train_raw(0, img=img)
    assert a['raw'] is enc and lc.same_value({k: v for k, v in a.items() if k != 'raw'}, {k: v for k, v in b.items() if k != 'raw'})


def test_single_gpu_test_gives_equal_results(small_dir, detector):
    """at the config's own scale, where the detector repeats itself bit for bit (tests/test_gpu_loader.py)"""
    data = lc.test_dataset(*small_dir, img_scale=demo_cases.IMG_SCALE)
    kw = dict(imgs_per_gpu=8, device_preprocess=True)
    rn.single_gpu_test(detector, data, workers=0, **kw)     # (a first pass over the shapes)
    want = rn.single_gpu_test(detector, data, workers=0, **kw)
    assert len(want) == 8 and sum(len(r) == 3 for r in want) > 0
    for workers in (0, 4):
        assert lc.same_value(rn.single_gpu_test(detector, data, workers=workers, device_decode=True, **kw), want)
    rows = rn.single_gpu_test(detector, data, workers=4, device_results=True, device_decode=True, **kw).to_host()
    assert lc.same_value(rows, rn.single_gpu_test(detector, data, workers=0, device_results=True, **kw).to_host())


def _rewrite(prefix, name, how):
    from PIL import Image
    path = os.path.join(prefix, name)
    if how == 'progressive':
        with Image.open(path) as im:
            im.save(path, quality=90, progressive=True)
        return
    with open(path, 'rb') as f:
        data = f.read()
    start = dr.scan_start(data)
    middle = start + (len(data) - start) // 2
    with open(path, 'wb') as f:
        f.write(data[:middle] + b'\xff\xd9' if how == 'corrupt' else data[:len(data) // 3])


def test_a_progressive_file_and_a_corrupted_scan_go_through_pil_with_a_warning_each(tmp_path):
    ann, prefix = lc.write_image_dir(str(tmp_path), n=8)
    data = lc.train_dataset(ann, prefix)
    names = [info['filename'] for info in data.img_infos]
    _rewrite(prefix, names[2], 'progressive')
    _rewrite(prefix, names[5], 'corrupt')
    assert 'progressive' in jpeg.parse_header(open(os.path.join(prefix, names[2]), 'rb').read())
    want, _ = epoch(data, 7, 2)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        got, _ = epoch(data, 7, 2, device_decode=True)
    assert_same_batches(got, want)
    messages = [str(w.message) for w in caught if 'JPEG decoder' in str(w.message)]
    assert len(messages) == 2, messages
    assert sum(names[2] in m and 'progressive' in m for m in messages) == 1
    assert sum(names[5] in m and 'status 3' in m for m in messages) == 1
    torch.cuda.synchronize()


def test_a_truncated_file_raises_what_the_pil_route_raises_at_its_batch(tmp_path):
    ann, prefix = lc.write_image_dir(str(tmp_path), n=8, truncate=5)
    data = lc.train_dataset(ann, prefix)
    assert not isinstance(jpeg.parse_header(open(os.path.join(prefix, data.img_infos[5]['filename']), 'rb').read()), str)

    def run(**kw):
        np.random.seed(2)
        taken = 0
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            with pytest.raises(Exception) as err:
                for _ in ld.build_dataloader(data, 2, 2, device='cuda', device_preprocess=True, **kw):
                    taken += 1
        return taken, err.type
    want = run()
    assert want[1] is OSError and run(device_decode=True) == want
    torch.cuda.synchronize()


def test_a_truncated_file_ends_the_epochs_threads_while_the_iterator_lives(tmp_path):
    """PIL's error comes out of the consumer's half of the route (the device refused the scan), not out of the pool: the
    epoch is closed there as it is for the pool's errors, not left to the iterator's collection"""
    import threading
    ann, prefix = lc.write_image_dir(str(tmp_path), n=8, truncate=5)
    data = lc.train_dataset(ann, prefix)
    np.random.seed(2)
    it = iter(ld.build_dataloader(data, 2, 2, device='cuda', device_preprocess=True, device_decode=True))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with pytest.raises(OSError):
            for _ in range(4):
                next(it)
    assert not [t.name for t in threading.enumerate() if t.name.startswith('kgdet-loader')]
    with pytest.raises(StopIteration):
        next(it)
    torch.cuda.synchronize()
