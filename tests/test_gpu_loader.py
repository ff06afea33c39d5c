"""kgdet_amd.loader and kgdet_amd.apis on the GPU: what the loader hands out on the device against the serial definition
(compared LATE, with every batch of the epoch kept alive: a ring slot refilled under its upload or a tensor handed out before
its stream was ordered shows as a wrong bit), ``train_detector`` end to end, the prefetching test loop, the inference entry
points and the two command-line tools.  JPEGs are written into tmp_path (tests/loader_cases.py)."""
import glob
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from kgdet_amd import apis
from kgdet_amd import datasets as ds
from kgdet_amd import loader as ld
from kgdet_amd import runner as rn
from kgdet_amd.checkpoint import save_checkpoint
from kgdet_amd.registry import Config
from tests import loader_cases as lc
from tests.golden import demo_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def _assert_on_device(batch, want_img, want_gt):
    assert batch['img'].is_cuda and batch['img'].dtype == torch.float32
    assert torch.equal(batch['img'], want_img)
    for key in GT_KEYS:
        assert len(batch[key]) == len(want_gt[key])
        for got, want in zip(batch[key], want_gt[key]):
            assert got.is_cuda and got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.cpu(), want)
    assert batch['gt_labels'][0].dtype == torch.int64


# ---- 1. device route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('busy', [False, True])
def test_device_route_equals_collate_device_when_compared_late(feed_dir, busy):
    data = lc.train_dataset(*feed_dir, img_scale=[(320, 256), (256, 192)], multiscale_mode='range', extra_aug=lc.EXTRA_AUG)
    np.random.seed(11)
    order = list(ds.GroupSampler(data, 2))
    serial = [[ld.draw_train_raw(data, i) for i in order[k:k + 2]] for k in range(0, len(order), 2)]
    state = np.random.get_state()
    a = torch.randn(2048, 2048, device='cuda') if busy else None

    np.random.seed(11)
    loader = ld.build_dataloader(data, 2, 4, device='cuda', device_preprocess=True, prefetch=3)
    kept = []
    for batch in loader:                      # the whole epoch is drawn and kept alive before anything is compared
        kept.append(batch)
        if busy:
            for _ in range(6):
                a = torch.mm(a, a).clamp_(-1, 1)
    assert len(kept) == len(serial) == len(loader) >= 6
    assert lc.same_rng_state(np.random.get_state(), state)
    transform = data.device_transform('cuda')
    for batch, samples in zip(kept, serial):
        want = ds.collate_device(samples, transform)
        _assert_on_device(batch, want['img'], want)
        assert lc.same_value(batch['img_meta'], want['img_meta'])
    torch.cuda.synchronize()


# ---- 2. host route with upload --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('workers', [0, 4])
def test_host_route_uploads_what_collate_makes(feed_dir, workers):
    data = lc.train_dataset(*feed_dir)
    np.random.seed(5)
    order = list(ds.GroupSampler(data, 2))
    serial = [ds.collate([data[i] for i in order[k:k + 2]]) for k in range(0, len(order), 2)]
    np.random.seed(5)
    kept = list(ld.build_dataloader(data, 2, workers, device='cuda:0', prefetch=3))
    assert len(kept) == len(serial)
    for batch, want in zip(kept, serial):
        _assert_on_device(batch, want['img'].cuda(), want)
        assert lc.same_value(batch['img_meta'], want['img_meta'])
    torch.cuda.synchronize()


# ---- 3. train_detector ----------------------------------------------------------------------------------------------------
def test_train_detector_runs_the_demo_config_and_its_first_step_is_the_serial_loops(small_dir, tmp_path):
    cfg = lc.demo_config(small_dir[0], small_dir[1], str(tmp_path / 'work'))
    data = ds.build_dataset(cfg['data']['train'])
    assert len(data) == 8
    lines = []
    np.random.seed(0)
    _, model = demo_cases.demo_detector()
    runner = apis.train_detector(model.cuda(), data, cfg, validate=True, logger=lines.append)
    assert runner.iter == 4 and runner.epoch == 1
    work = str(tmp_path / 'work')
    assert os.path.isfile(os.path.join(work, 'epoch_1.pth')) and os.path.isfile(os.path.join(work, 'latest.pth'))
    logs = glob.glob(os.path.join(work, '*.log.json'))
    assert len(logs) == 1
    with open(logs[0]) as f:
        records = [json.loads(line) for line in f]
    train = [r for r in records if r['mode'] == 'train']
    val = [r for r in records if r['mode'] == 'val']
    assert len(train) == 4 and [r['iter'] for r in train] == [1, 2, 3, 4]
    assert all(r['data_time'] >= 0 and r['time'] >= r['data_time'] for r in train)
    assert len(val) == 1 and 'bbox_mAP' in val[0] and 'keypoints_mAP' in val[0]
    names = [k for k in train[0] if k.startswith('loss_')]
    assert len(names) == 9
    assert all(np.isfinite(r[k]) for r in train for k in names + ['loss'])

    # the first step, from the serial definition under the same seed: same weights, same batch -> the same nine losses
    np.random.seed(0)
    order = list(ds.GroupSampler(data, 2))
    first = ds.collate([data[i] for i in order[:2]])
    first['img'] = first['img'].cuda()
    for key in GT_KEYS:
        first[key] = [t.cuda() for t in first[key]]
    _, model2 = demo_cases.demo_detector()
    model2 = model2.cuda()
    serial = rn.Runner(model2, rn.build_optimizer(model2, cfg['optimizer']), lr_config=cfg['lr_config'],
                       optimizer_config=cfg['optimizer_config'], log_interval=1, logger=lambda s: None)
    serial.run([first], max_epochs=1)
    for k in names:
        assert serial.log_history[0][k] == runner.log_history[0][k] == train[0][k], k


# ---- 4. the prefetching test loop -----------------------------------------------------------------------------------------
def _some_detections(results):
    return sum(len(r) == 3 for r in results) > 0


@pytest.mark.parametrize('device_preprocess', [False, True])
def test_single_gpu_test_with_workers_equals_without(small_dir, detector, device_preprocess):
    """At the config's own scale, not the small one: equality of RESULTS needs a detector that repeats itself bit for bit, and at
    (320, 256) this one does not -- measured on an MI355X, ``workers=0`` against ``workers=0`` on bit-equal inputs (hashed), either
    route, ``imgs_per_gpu`` 1 and 2: the boxes of the one image with detections differ by 1.5e-5 to 6.1e-5 from run to run.  At
    (1333, 800) the suite already holds the detector to array-for-array repeats (tests/test_gpu_preprocess.py)."""
    data = lc.test_dataset(*small_dir, img_scale=demo_cases.IMG_SCALE)
    kw = dict(to_device=lambda t: t.cuda(), imgs_per_gpu=8, device_preprocess=device_preprocess)
    # (a first pass over the shapes: the first forward at a new shape may pick other convolution algorithms)
    rn.single_gpu_test(detector, data, workers=0, **kw)
    want = rn.single_gpu_test(detector, data, workers=0, **kw)
    got = rn.single_gpu_test(detector, data, workers=4, **kw)
    assert len(want) == 8 and _some_detections(want) and lc.same_value(got, want)
    rows_want = rn.single_gpu_test(detector, data, workers=0, device_results=True, **kw).to_host()
    rows_got = rn.single_gpu_test(detector, data, workers=4, device_results=True, **kw).to_host()
    assert lc.same_value(rows_got, rows_want)


# ---- 5. init_detector + inference_detector --------------------------------------------------------------------------------
def test_init_and_inference_detector_equal_single_gpu_test(small_dir, detector, tmp_path):
    """(at the config's own scale, for the reason given in the test above)"""
    cfg = Config(lc.demo_config(small_dir[0], small_dir[1], None, img_scale=demo_cases.IMG_SCALE))
    ckpt = str(tmp_path / 'demo.pth')
    save_checkpoint(detector, ckpt)
    model = apis.init_detector(cfg, ckpt, device='cuda:0')
    assert not model.training and model.cfg is cfg
    data = lc.test_dataset(*small_dir, img_scale=demo_cases.IMG_SCALE)
    rn.single_gpu_test(model, data, to_device=lambda t: t.cuda())        # (a first pass over the shapes, as above)
    want = rn.single_gpu_test(model, data, to_device=lambda t: t.cuda())
    assert _some_detections(want)
    paths = [os.path.join(small_dir[1], info['filename']) for info in data.img_infos]
    got = apis.inference_detector(model, paths)
    assert len(got) == 8 and lc.same_value(got, want)
    assert lc.same_value(apis.inference_detector(model, paths[1]), want[1])
    rn.single_gpu_test(model, data, device_preprocess=True)
    want_dev = rn.single_gpu_test(model, data, device_preprocess=True)
    assert lc.same_value(apis.inference_detector(model, paths, device_preprocess=True), want_dev)


# ---- the command lines ----------------------------------------------------------------------------------------------------
def _tool(name):
    spec = importlib.util.spec_from_file_location('kgdet_tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_train_and_test_tools_run_a_config_file_to_the_end(small_dir, tmp_path):
    work = str(tmp_path / 'work')
    config = lc.write_config_file(str(tmp_path / 'demo_small.py'), lc.demo_config(small_dir[0], small_dir[1], work))
    _tool('train').main([config, '--validate', '--seed', '0', '--device-preprocess'])
    ckpt = os.path.join(work, 'latest.pth')
    assert os.path.isfile(ckpt) and len(glob.glob(os.path.join(work, '*.log.json'))) == 1
    out = str(tmp_path / 'res')
    stats = _tool('test').main([config, ckpt, '--json_out', out, '--eval', 'bbox', 'keypoints', '--workers', '4',
                                '--imgs-per-gpu', '2'])
    assert os.path.isfile(out + '.bbox.json') and os.path.isfile(out + '.keypoints.json')
    assert set(stats) == {'bbox', 'keypoints'} and all(np.isfinite(np.asarray(stats[t])).all() for t in stats)
    direct = _tool('test').main([config, ckpt, '--eval', 'bbox', 'keypoints', '--device-preprocess', '--device-results',
                                 '--imgs-per-gpu', '2'])
    assert set(direct) == {'bbox', 'keypoints'}
    with pytest.raises(SystemExit):
        _tool('test').main([config, ckpt, '--eval', 'bbox', '--launcher', 'pytorch'])
    with pytest.raises(SystemExit):
        _tool('train').main([config, '--launcher', 'slurm'])
