"""The whole-batch decode (kgdet_amd/decode.py) of both head families against tests/golden/decode_golden.npz: what
``get_bboxes(..., nms=False)`` returned, on the CPU and on the GPU, at the commit stored in the fixture -- the last one with the
reference's per-image, per-level decode loops (tests/golden/make_decode_golden.py makes the inputs and names the cases).

Candidate order, boxes and landmarks must be bit-equal.  Scores must be bit-equal on the GPU and within one float32 ulp on
the CPU, where the rounding of ``sigmoid`` depends on an element's position in its tensor; the fixture's generator keeps such a
difference from changing the selection."""
import os

import numpy as np
import pytest
import torch

from tests.golden import make_decode_golden as gen

NAMES = [c[0] for c in gen.CASES]


@pytest.fixture(scope='module')
def golden():
    data = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'decode_golden.npz'))
    assert len(str(data['commit:cpu'])) == 40 and str(data['commit:cpu']) == str(data['commit:cuda'])
    return data


def _check(golden, name, device, scores):
    """scores: None = all but the scores, bit-equal; 0 = the scores, bit-equal; n = the scores, within n ulps of the recording"""
    got = gen.run_case(name, device)
    want = {k[len(device) + 1:]: golden[k] for k in golden.files if k.startswith('%s:%s:' % (device, name))}
    assert want and sorted(got) == sorted(want)
    if name == 'kgdet_per_axis':        # a 4-vector does not divide the landmarks' (x, y): RuntimeError before and after
        assert list(got) == [name + ':raises']
        return
    assert len(got) == 4 * len(gen.IMG_SHAPES)
    for key, w in want.items():
        g = got[key]
        if key.endswith(':scores') != (scores is not None):
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, key
        if scores:
            ulps = np.abs(g.astype(np.float64) - w) / np.spacing(np.abs(w)).astype(np.float64)
            print(key, 'scores that differ:', int((g != w).sum()), 'of', g.size, 'by at most', float(ulps.max()), 'ulps')
            assert ulps.max() <= scores, key
        else:
            assert np.array_equal(g, w), key


def test_fixture_covers_every_rule(golden):
    """the recorded candidates do leave the images (so every clamp acts), both levels are cut, and the two rescale rules and
    the two clamp axes are visible in the recording itself"""
    for dev in ('cpu', 'cuda'):
        for i, (h, w, _) in enumerate(gen.IMG_SHAPES):
            b = golden['%s:kgdet_plain:%d:bboxes' % (dev, i)]
            assert b.shape == (2 * gen.NMS_PRE, 4) and b.min() == 0 and b[:, 0::2].max() == w and b[:, 1::2].max() == h
            k = golden['%s:kgdet_plain:%d:kpts' % (dev, i)]
            assert k[..., 0].max() == w and k[..., 1].max() == h and k[..., :2].min() == 0
            s = golden['%s:serial_plain:%d:kpts' % (dev, i)]       # landmarks 0, 3, .. to W; 1, 4, .. to H; 2, 5, .. free
            assert s[:, 0::3, :2].max() == w and s[:, 1::3, :2].max() == h and s[:, 2::3, :2].max() > max(h, w)
            assert tuple(golden['%s:kgdet_plain:%d:kpts_shape' % (dev, i)]) == (2 * gen.NMS_PRE, gen.K, 3)
            assert tuple(golden['%s:kgdet_rescale:%d:kpts_shape' % (dev, i)]) == (2 * gen.NMS_PRE, 3 * gen.K)
    # division by a python number is a multiplication with the reciprocal on the GPU only; by a tensor it is true everywhere
    a, b = (golden['%s:kgdet_rescale:1:bboxes' % d] for d in ('cpu', 'cuda'))
    assert not np.array_equal(a, b)
    a, b = (golden['%s:kgdet_np_factor:1:bboxes' % d] for d in ('cpu', 'cuda'))
    assert np.array_equal(a, b)


@pytest.mark.parametrize('name', NAMES)
def test_decode_matches_the_recording_cpu(golden, name):
    """candidate order, boxes, landmarks and shapes: bit-equal"""
    _check(golden, name, 'cpu', None)


@pytest.mark.parametrize('name', NAMES)
def test_decode_scores_within_one_ulp_of_the_recording_cpu(golden, name):
    """The bar is one float32 ulp (``np.spacing``) of the recorded score.  ``decode.class_scores`` keeps an image's scores
    independent of the batch on the CPU as well (torch's vector and scalar ``sigmoid`` routines differ by up to two ulps, and
    which elements take the scalar one depends on the tensor's size), so the recording is met bit for bit; each case prints
    how many scores differ."""
    _check(golden, name, 'cpu', 1)


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_decode_matches_the_recording_gpu(golden, name):
    """everything, scores included: bit-equal"""
    _check(golden, name, 'cuda', None)
    _check(golden, name, 'cuda', 0)
