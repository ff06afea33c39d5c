"""kgdet_amd.loader on the CPU: the threaded feed against the serial loop it is defined by (bit for bit, RNG state included),
its failure and shutdown paths, its lookahead bound, and the prefetch of the test loops.  Images are JPEGs the tests write
into tmp_path (tests/loader_cases.py).  The failure and lookahead tests come first: a loader bug has to show as a failed
assertion, never as a hang."""
import threading
import time

import numpy as np
import pytest
import torch

from kgdet_amd import datasets as ds
from kgdet_amd import loader as ld
from kgdet_amd import runner as rn
from tests import loader_cases as lc


def _threads_back_to(before, within=5.0):
    end = time.time() + within
    while time.time() < end:
        if set(threading.enumerate()) <= before:
            return True
        time.sleep(0.01)
    return False


@pytest.fixture(scope='module')
def image_dir(tmp_path_factory):
    return lc.write_image_dir(str(tmp_path_factory.mktemp('feed')), n=8, no_anno=2)


@pytest.fixture(scope='module')
def plain_dir(tmp_path_factory):
    return lc.write_image_dir(str(tmp_path_factory.mktemp('plain')), n=8)


# ---- 4. failure -------------------------------------------------------------------------------------------------------
def test_a_decoder_error_arrives_at_its_batch_with_its_type_and_every_thread_ends(tmp_path):
    ann, prefix = lc.write_image_dir(str(tmp_path), n=8, truncate=5)
    data = lc.train_dataset(ann, prefix)
    with pytest.raises(Exception) as serial:           # the decoder's own exception, as the serial loop meets it
        data.load_image(5)
    before = set(threading.enumerate())
    loader = ld.build_dataloader(data, 2, 4, shuffle=False, prefetch=3)
    got = []
    with pytest.raises(serial.type):
        for batch in loader:
            got.append(batch)
    assert len(got) == 2                               # images 0-3 arrive; the batch of images 4 and 5 raises
    assert [m['ori_shape'] for b in got for m in b['img_meta']] == \
        [(data.img_infos[i]['height'], data.img_infos[i]['width'], 3) for i in range(4)]
    assert _threads_back_to(before)


def test_break_close_and_garbage_collection_end_every_thread(image_dir):
    data = lc.train_dataset(*image_dir)
    before = set(threading.enumerate())
    loader = ld.build_dataloader(data, 2, 4, shuffle=False, prefetch=2)
    for batch in loader:
        break
    assert _threads_back_to(before)                    # the for statement dropped the iterator
    it = iter(loader)
    next(it)
    assert not set(threading.enumerate()) <= before
    loader.close()
    assert _threads_back_to(before)
    with pytest.raises(StopIteration):
        next(it)
    it = iter(loader)
    next(it)
    del it, loader
    assert _threads_back_to(before)


def test_a_failure_in_the_pixel_work_wakes_the_consumer(image_dir):
    data = lc.train_dataset(*image_dir)

    class Boom(RuntimeError):
        pass

    calls = []

    def transform(img, scale, flip=False, keep_ratio=True, inner=data.img_transform):
        calls.append(1)
        if len(calls) == 4:
            raise Boom('pixel work')
        return inner(img, scale, flip, keep_ratio=keep_ratio)

    data.img_transform = transform
    before = set(threading.enumerate())
    t0 = time.time()
    with pytest.raises(Boom):
        list(ld.build_dataloader(data, 2, 2, shuffle=False))
    assert time.time() - t0 < 5 and _threads_back_to(before)


# ---- 5. bounded lookahead -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('workers,prefetch', [(1, 1), (4, 2)])
def test_decodes_never_run_further_ahead_than_the_window(plain_dir, workers, prefetch):
    data = lc.train_dataset(*plain_dir)
    B, consumed, worst, lock = 2, [0], [0], threading.Lock()
    inner = data.load_image

    def load_image(idx):
        with lock:                                      # (shuffle=False: the index IS the place in the order)
            worst[0] = max(worst[0], idx + 1 - consumed[0])
        return inner(idx)

    data.load_image = load_image
    for batch in ld.build_dataloader(data, B, workers, shuffle=False, prefetch=prefetch):
        with lock:
            consumed[0] += len(batch['img'])
        time.sleep(0.05)                                # a slow consumer: the producers run into their bound
    assert consumed[0] == len(data)
    assert 0 < worst[0] <= prefetch * B + workers


# ---- 1. / 2. serial equivalence -----------------------------------------------------------------------------------------
def _serial_epochs(data, B, raw, epochs, seed):
    """the definition: iter(sampler), then dataset[i] (prepare_train_raw + the resample for the raw route), then collate"""
    np.random.seed(seed)
    out = []
    for _ in range(epochs):
        order = list(ds.GroupSampler(data, B))
        if raw:
            batches = [[ld.draw_train_raw(data, i) for i in order[k:k + B]] for k in range(0, len(order), B)]
        else:
            batches = [ds.collate([data[i] for i in order[k:k + B]]) for k in range(0, len(order), B)]
        out.append((order, batches))
    return out, np.random.get_state()


@pytest.fixture(scope='module')
def aug_dataset(image_dir):
    return lc.train_dataset(*image_dir, img_scale=[(320, 256), (256, 192)], multiscale_mode='range', extra_aug=lc.EXTRA_AUG)


@pytest.fixture(scope='module')
def serial_host(aug_dataset):
    return _serial_epochs(aug_dataset, 2, False, 2, seed=7)


@pytest.fixture(scope='module')
def serial_raw(aug_dataset):
    return _serial_epochs(aug_dataset, 2, True, 2, seed=7)


def test_the_case_runs_the_resample_path_and_reorders_between_epochs(aug_dataset, serial_host):
    assert aug_dataset.prepare_train_raw(2) is None and len(aug_dataset) == 8
    (order0, _), (order1, _) = serial_host[0]
    assert 2 in order0 and order0 != order1


@pytest.mark.parametrize('workers', [0, 1, 4])
@pytest.mark.parametrize('prefetch', [1, 3])
def test_host_route_equals_the_serial_loop_bit_for_bit(aug_dataset, serial_host, workers, prefetch):
    epochs, state = serial_host
    np.random.seed(7)
    loader = ld.build_dataloader(aug_dataset, 2, workers, prefetch=prefetch)
    assert len(loader) == len(epochs[0][1])
    for _, want in epochs:
        got = list(loader)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert list(g.keys()) == list(w.keys())
            assert lc.same_value(g, w)
    assert lc.same_rng_state(np.random.get_state(), state)


@pytest.mark.parametrize('workers', [0, 1, 4])
@pytest.mark.parametrize('prefetch', [1, 3])
def test_raw_route_equals_prepare_train_raw_with_its_aug_plans(aug_dataset, serial_raw, workers, prefetch):
    epochs, state = serial_raw
    np.random.seed(7)
    loader = ld.build_dataloader(aug_dataset, 2, workers, prefetch=prefetch, device_preprocess=True)
    for _, want in epochs:
        got = list(loader)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert all('aug_plan' in s for s in g)
            assert lc.same_value(g, w)
    assert lc.same_rng_state(np.random.get_state(), state)


def test_finish_train_sample_is_prepare_train_img(aug_dataset):
    np.random.seed(3)
    want = aug_dataset.prepare_train_img(0)
    np.random.seed(3)
    got = ds.finish_train_sample(aug_dataset, aug_dataset.prepare_train_raw(0))
    assert list(got.keys()) == list(want.keys()) and lc.same_value(got, want)


# ---- 3. dataset order, short batch, set_epoch -----------------------------------------------------------------------------
def test_dataset_order_short_last_batch_and_set_epoch(plain_dir):
    data = lc.train_dataset(*plain_dir, flip_ratio=0)
    loader = ld.build_dataloader(data, 3, 2, shuffle=False)
    assert len(loader) == 3
    got = list(loader)
    assert [len(b['img']) for b in got] == [3, 3, 2]
    want = [ds.collate([data[i] for i in idx]) for idx in ([0, 1, 2], [3, 4, 5], [6, 7])]
    assert lc.same_value(got, want)

    sampler = ds.DistributedGroupSampler(data, 2, num_replicas=2, rank=1)
    loader = ld.build_dataloader(data, 2, 2, sampler=sampler)
    assert len(loader) == len(sampler) // 2
    orders = []
    for epoch in (0, 1):
        loader.set_epoch(epoch)
        assert sampler.epoch == epoch
        order = list(sampler)
        orders.append(order)
        got = list(loader)
        want = [ds.collate([data[i] for i in order[k:k + 2]]) for k in range(0, len(order), 2)]
        assert lc.same_value(got, want)
    assert orders[0] != orders[1]


# ---- 6. test-loop prefetch ------------------------------------------------------------------------------------------------
class _Recorder(torch.nn.Module):
    """a detector stub: records what it is called with; one result per image derived from the pixels"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def forward(self, imgs, metas, return_loss=False, rescale=False):
        self.calls.append(('forward', [t.clone() for t in imgs], metas, rescale))
        return [np.array([float(sum(t.sum() for t in imgs))], dtype=np.float32)]

    def simple_test_batch(self, img, metas, rescale=False):
        self.calls.append(('batch', img.clone(), metas, rescale))
        return [[np.array([float(t.sum())], dtype=np.float32)] for t in img]


@pytest.mark.parametrize('tta', [False, True])
@pytest.mark.parametrize('imgs_per_gpu', [1, 3])
def test_test_loop_prefetch_makes_the_same_calls_in_the_same_order(image_dir, tta, imgs_per_gpu):
    kw = dict(img_scale=[(320, 256), (256, 192)], flip_ratio=0.5) if tta else {}
    data = lc.test_dataset(*image_dir, **kw)
    before = set(threading.enumerate())
    plain, ahead = _Recorder(), _Recorder()
    want = rn.single_gpu_test(plain, data, imgs_per_gpu=imgs_per_gpu, workers=0)
    got = rn.single_gpu_test(ahead, data, imgs_per_gpu=imgs_per_gpu, workers=4)
    assert len(want) == len(data) and lc.same_value(got, want)
    assert len(plain.calls) == len(ahead.calls) and lc.same_value(ahead.calls, plain.calls)
    assert (len(plain.calls[0][1]) == 4) if tta else (imgs_per_gpu == 1 or any(c[0] == 'batch' for c in plain.calls))
    assert _threads_back_to(before)


def test_test_loop_prefetch_raises_the_decoders_exception(tmp_path):
    ann, prefix = lc.write_image_dir(str(tmp_path), n=8, truncate=3)
    data = lc.test_dataset(ann, prefix)
    with pytest.raises(Exception) as serial:
        data.load_image(3)
    before = set(threading.enumerate())
    with pytest.raises(serial.type):
        rn.single_gpu_test(_Recorder(), data, workers=4)
    assert _threads_back_to(before)


# ---- 7. argument checks ---------------------------------------------------------------------------------------------------
def test_argument_checks(image_dir):
    data = lc.train_dataset(*image_dir)
    with pytest.raises(ValueError):
        ld.build_dataloader(data, 2, -1)
    with pytest.raises(ValueError):
        ld.build_dataloader(data, 2, 2, prefetch=-1)
    with pytest.raises(ValueError):
        rn.single_gpu_test(_Recorder(), lc.test_dataset(*image_dir), workers=-1)
    assert ld.build_dataloader(data, 2, 64).workers == 16
    assert ld.build_dataloader(data, 2, 12, num_gpus=2).workers == 16
    with pytest.raises(ValueError):
        ld.build_dataloader(data, 2, 2, device='cpu')
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            ld.build_dataloader(data, 2, 2, device='cuda:0')
