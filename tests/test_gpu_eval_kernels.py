"""``kgdet_coco_similarity`` and ``kgdet_coco_match`` (csrc/coco_eval.hip) through the C ABI against the scalar references of
tests/eval_kernel_cases.py, at the lane and wave counts and the decisions that whole evaluations (tests/test_gpu_eval.py) keep
clear of by construction.

Bars: IoU bit-equal; OKS within a relative 1e-12 (the bar and derivation of tests/test_gpu_eval.py: bit-identical exponent
argument, each library's float64 exp good to a few ulp, at most 294 non-negative terms in another order), and EXACTLY 1.0 /
0.0 where every exponent argument is 0 / above 746; matching outputs equal -- the similarity matrix is an input there, written
by hand, so nothing sits near a decision.  Every output is a view between canaries, prefilled: rows and words of skipped cells
must keep the fill.  Every launch runs twice into fresh buffers."""
import ctypes

import numpy as np
import pytest
import torch

from kgdet_amd import _lib
from tests import eval_kernel_cases as E

pytestmark = pytest.mark.gpu
PAD = 64
i32, i64 = ctypes.c_int32, ctypes.c_int64
CANARY = {np.dtype(np.float64): -12345.5, np.dtype(np.int32): -777, np.dtype(np.uint8): 0x5A}


class Out(object):
    """an output array between canaries in a buffer of its own, prefilled with ``fill``"""

    def __init__(self, shape, dtype, fill):
        self.shape, self.n, self.dtype = shape, int(np.prod(shape)), np.dtype(dtype)
        host = np.full(self.n + 2 * PAD, CANARY[self.dtype], dtype=self.dtype)
        host[PAD:PAD + self.n] = fill
        self.buf = torch.from_numpy(host).cuda()

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + PAD * self.dtype.itemsize)

    def read(self):
        host = self.buf.cpu().numpy()
        assert (host[:PAD] == CANARY[self.dtype]).all() and (host[PAD + self.n:] == CANARY[self.dtype]).all(), 'a canary was overwritten'
        return host[PAD:PAD + self.n].reshape(self.shape).copy()


def _up(a, dtype):
    """an input on the device; an empty one still gets an address (one element), so that only the sizes say it is empty"""
    a = np.ascontiguousarray(np.asarray(a).astype(dtype, copy=False))
    return torch.from_numpy(a if a.size else np.zeros(1, dtype)).cuda()


def _similarity(c):
    kp = c.iou_type == 'keypoints'
    p = _lib.ptr
    dev = dict(cells=_up(c.cells, np.int32), off=_up(c.sim_off, np.int64), d_box=_up(c.d_box, np.float64), d_kxy=_up(c.d_kxy, np.float64),
               g_box=_up(c.g_box, np.float64), g_kpt=_up(c.g_kpt, np.float64), g_area=_up(c.g_area, np.float64),
               g_crowd=_up(c.g_crowd, np.int32), g_nvis=_up(c.g_nvis, np.int32), var=_up(c.var, np.float64))
    sim = Out((c.sim_size, ), np.float64, E.FILL_SIM)
    rc = _lib.lib().kgdet_coco_similarity(i32(1 if kp else 0), p(dev['cells']), p(dev['off']), i32(len(c.cells)), i64(c.nd), i64(c.ng),
                                          i64(c.sim_size), p(dev['d_box']), p(dev['d_kxy']), p(dev['g_box']), p(dev['g_kpt']),
                                          p(dev['g_area']), p(dev['g_crowd']), p(dev['g_nvis']), p(dev['var']), i32(c.K), sim.ptr(),
                                          _lib.current_stream())
    assert rc == _lib.KGDET_OK, _lib.lib().kgdet_last_error()
    torch.cuda.synchronize()
    return sim.read()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_box_iou_is_bit_equal():
    c = E.iou_case()
    want = E.reference_similarity(c)
    got, again = _similarity(c), _similarity(c)
    assert _same_bits(got, again)
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert not bad.size, (bad[:8], got[bad[:8]], want[bad[:8]])
    assert np.isnan(want).sum() > 0                                   # (the reserved words of the skipped cells: fill on both sides)


@pytest.mark.parametrize('K', E.SIM_KS)
def test_oks_within_the_bar_and_exact_where_it_must_be(K):
    c = E.oks_case(K)
    want = E.reference_similarity(c)
    got, again = _similarity(c), _similarity(c)
    assert _same_bits(got, again)
    fill = np.array([E.FILL_SIM]).view(np.uint64)[0]
    skipped = want.view(np.uint64) == fill
    assert skipped.any() and np.array_equal(got.view(np.uint64) == fill, skipped), 'a skipped cell was written, or a word of a valid one was not'
    g, w = got[~skipped], want[~skipped]
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(w != 0, np.abs(g - w) / np.abs(w), np.abs(g))
    worst = float(rel.max())
    print('OKS K = %d: %d values, worst relative difference %.3e' % (K, g.size, worst))
    assert worst <= 1e-12
    n = 0
    for off, ones, zeros, _ in E.oks_arguments(c):
        block = got[off:off + ones.size].reshape(ones.shape)
        assert (block[ones] == 1.0).all() and (block[zeros] == 0.0).all()
        assert not np.signbit(block[zeros]).any()
        n += int(ones.sum()) + int(zeros.sum())
    assert n >= 7


def test_similarity_with_no_cell_writes_nothing():
    c = E.iou_case()
    sim = Out((c.sim_size, ), np.float64, E.FILL_SIM)
    z = ctypes.c_void_p(0)
    for typ in (0, 1):
        rc = _lib.lib().kgdet_coco_similarity(i32(typ), z, z, i32(0), i64(c.nd), i64(c.ng), i64(c.sim_size), z, z, z, z, z, z, z, z,
                                              i32(1), sim.ptr(), _lib.current_stream())
        assert rc == _lib.KGDET_OK
    torch.cuda.synchronize()
    assert (sim.read().view(np.uint64) == np.array([E.FILL_SIM]).view(np.uint64)[0]).all()


# --- matching ------------------------------------------------------------------------------------------------------------------
def _match(c, A=None, T=None, expect=_lib.KGDET_OK):
    A, T = (c.A if A is None else A), (c.T if T is None else T)
    p = _lib.ptr
    dev = dict(cells=_up(c.cells, np.int32), off=_up(c.sim_off, np.int64), sim=_up(c.sim, np.float64), d_area=_up(c.d_area, np.float64),
               g_area=_up(c.g_area, np.float64), g_ign=_up(c.g_ign, np.uint8), g_crowd=_up(c.g_crowd, np.int32),
               rng=_up(np.resize(c.area_rng, (A, 2)), np.float64), best0=_up(np.resize(c.best0, T), np.float64))
    outs = (Out((c.nd, A, T), np.int32, E.FILL_I32), Out((c.nd, A, T), np.uint8, E.FILL_U8), Out((c.ng, A), np.uint8, E.FILL_U8),
            Out((c.ng, A, T), np.uint8, 0xFF))                        # (g_taken: scratch, handed over dirty)
    rc = _lib.lib().kgdet_coco_match(p(dev['cells']), p(dev['off']), i32(len(c.cells)), i64(c.nd), i64(c.ng), i64(c.sim_size),
                                     p(dev['sim']), p(dev['d_area']), p(dev['g_area']), p(dev['g_ign']), p(dev['g_crowd']),
                                     p(dev['rng']), i32(A), p(dev['best0']), i32(T), outs[0].ptr(), outs[1].ptr(), outs[2].ptr(),
                                     outs[3].ptr(), _lib.current_stream())
    assert rc == expect, (rc, _lib.lib().kgdet_last_error())
    torch.cuda.synchronize()
    return [o.read() for o in outs]


@pytest.mark.parametrize('A,T', E.MATCH_SHAPES)
def test_matcher_equals_the_scalar_loop(A, T):
    c = E.match_case(A, T)
    want = E.reference_match(c)
    got, again = _match(c), _match(c)
    for name, g, g2, w in zip(('d_match', 'd_ignore', 'g_ignore_out'), got, again, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        bad = np.argwhere(g != w)
        assert not bad.size, '%s: %d differ, first at %s: %s against %s' % (name, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])])
        assert np.array_equal(g, g2), name
    rows_d, rows_g = E.written_rows(c)
    assert (got[0][~rows_d] == E.FILL_I32).all() and (got[2][~rows_g] == E.FILL_U8).all()      # skipped cells: rows left alone
    assert (got[3][~rows_g] == 0xFF).all()


def test_more_lanes_than_a_wave_are_refused_and_nothing_is_written():
    c = E.match_case(4, 16)
    got = _match(c, A=5, T=13, expect=_lib.KGDET_E_SHAPE)
    assert b'lanes' in _lib.lib().kgdet_last_error()
    assert (got[0] == E.FILL_I32).all() and (got[1] == E.FILL_U8).all() and (got[2] == E.FILL_U8).all() and (got[3] == 0xFF).all()
