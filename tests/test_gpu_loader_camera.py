"""``device_decode='camera'`` on the GPU: ``build_dataloader`` and ``single_gpu_test`` on a set that holds 4:2:2 files and files
with restart intervals, against the same calls with ``device_decode=False`` -- bit for bit and without a warning, since
``kgdet_jpeg_decode_camera``'s pictures are PIL's --; ``device_decode=True`` on the same set (the same batches, one warning per
such file); and a file whose restart markers are out of turn, which the kernels refuse and PIL decodes.  JPEGs are written
into tmp_path (tests/loader_cases.py's rendered records) and re-saved with PIL."""
import os
import warnings

import pytest
import torch

from kgdet_amd import jpeg
from kgdet_amd import runner as rn
from tests import jpeg_camera_refs as cr
from tests import loader_cases as lc
from tests.golden import demo_cases
from tests.test_gpu_loader_decode import assert_same_batches, epoch

pytestmark = pytest.mark.gpu
RESAVED = {1: dict(subsampling='4:2:2'), 4: dict(subsampling='4:2:2', restart_marker_blocks=7), 2: dict(restart_marker_rows=1),
           6: dict(restart_marker_rows=1, subsampling='4:4:4')}


def camera_dir(root):
    """8 rendered records, two of them re-saved as 4:2:2 (one with an interval that divides no row) and two with one-row intervals
    -> (annotations, prefix, the names of the four)"""
    from PIL import Image
    ann, prefix = lc.write_image_dir(root, n=8)
    names = [info['filename'] for info in lc.train_dataset(ann, prefix).img_infos]
    for k, how in RESAVED.items():
        path = os.path.join(prefix, names[k])
        with Image.open(path) as im:
            im.load()
            im.save(path, 'JPEG', quality=90, **how)
        frame = jpeg.parse_header(open(path, 'rb').read(), camera=True)
        assert (frame['mode'] == jpeg.MODE_422) == (how.get('subsampling') == '4:2:2')
        assert (frame['restart_interval'] > 0) == any(key.startswith('restart') for key in how)
        assert isinstance(jpeg.parse_header(open(path, 'rb').read()), str)
    return ann, prefix, [names[k] for k in sorted(RESAVED)]


@pytest.fixture(scope='module')
def feed(tmp_path_factory):
    return camera_dir(str(tmp_path_factory.mktemp('camera')))


def test_the_loader_yields_the_same_batches_without_a_warning(feed):
    ann, prefix, _ = feed
    data = lc.train_dataset(ann, prefix, img_scale=[(320, 256), (256, 192)], multiscale_mode='range', extra_aug=lc.EXTRA_AUG)
    want, state = epoch(data, 11, 2)
    with warnings.catch_warnings():
        warnings.simplefilter('error')                      # every file is one the camera route takes: nothing falls back
        got, state_camera = epoch(data, 11, 2, device_decode='camera')
        serial, _ = epoch(data, 11, 0, device_decode='camera')
    assert lc.same_rng_state(state_camera, state)
    assert_same_batches(got, want)
    assert_same_batches(serial, want)
    torch.cuda.synchronize()


def test_the_baseline_route_decodes_such_files_on_the_host_with_one_warning_each(feed):
    ann, prefix, resaved = feed
    data = lc.train_dataset(ann, prefix)
    want, _ = epoch(data, 5, 2)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        got, _ = epoch(data, 5, 2, device_decode=True)
    assert_same_batches(got, want)
    messages = [str(w.message) for w in caught if 'JPEG decoder' in str(w.message)]
    assert len(messages) == 4 and all(sum(name in m for m in messages) == 1 for name in resaved), messages
    assert sum('sampling 2x1' in m for m in messages) == 1 and sum('restart interval' in m for m in messages) == 3
    with pytest.raises(ValueError, match="'camera'"):
        epoch(data, 5, 0, device_decode='cameras')
    torch.cuda.synchronize()


def test_single_gpu_test_gives_equal_results(feed):
    """at the config's own scale, where the detector repeats itself bit for bit (tests/test_gpu_loader.py)"""
    ann, prefix, _ = feed
    _, model = demo_cases.demo_detector()
    detector = model.cuda().eval()
    data = lc.test_dataset(ann, prefix, img_scale=demo_cases.IMG_SCALE)
    kw = dict(imgs_per_gpu=8, device_preprocess=True)
    rn.single_gpu_test(detector, data, workers=0, **kw)     # (a first pass over the shapes)
    want = rn.single_gpu_test(detector, data, workers=0, **kw)
    assert len(want) == 8
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        for workers in (0, 4):
            assert lc.same_value(rn.single_gpu_test(detector, data, workers=workers, device_decode='camera', **kw), want)


def test_a_file_with_a_swapped_restart_marker_goes_through_pil_with_one_warning(tmp_path):
    ann, prefix, resaved = camera_dir(str(tmp_path))
    path = os.path.join(prefix, resaved[1])                 # (one-row intervals)
    good = open(path, 'rb').read()
    with open(path, 'wb') as f:
        f.write(cr.broken(good)['swapped'])
    data = lc.train_dataset(ann, prefix)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                     # (libjpeg's own complaint about the markers)
        want, _ = epoch(data, 7, 2)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        got, _ = epoch(data, 7, 2, device_decode='camera')
    assert_same_batches(got, want)
    messages = [str(w.message) for w in caught if 'JPEG decoder' in str(w.message)]
    assert len(messages) == 1 and resaved[1] in messages[0] and 'status 4' in messages[0], messages
    torch.cuda.synchronize()
