"""``kgdet_aug_merge`` (csrc/aug_merge.hip) through the C ABI against the numpy references of tests/aug_merge_cases.py, at the
row widths, row counts and pointer offsets where its staging takes another path (the table there names which), and
``postprocess.aug_merge_kp`` on the inputs its callers may hand it.

Bars: the bits of ``reference_f32`` (NaN payloads, infinities, -0.0 and subnormals in the copied fields included), and the
counted bound of ``reference_f64`` (derivation in the cases file).  Every output is a view inside a buffer of CANARY words,
prefilled with one NaN bit pattern that no input carries: an element the kernel skipped and a write beside the view both show.
Every launch runs twice into fresh buffers."""
import ctypes

import numpy as np
import pytest
import torch

from kgdet_amd import _lib
from tests import aug_merge_cases as M

pytestmark = pytest.mark.gpu

CANARY, FILL = 0x4b1dc0de, 0x7fc5a5a5        # (int32 words; FILL is a quiet NaN with a payload of its own)
PAD = 64                                     # words either side; a multiple of 4, so the offset alone sets the alignment
i32 = ctypes.c_int32


class Block(object):
    """``n`` float32 words at ``off`` words past a 16-byte boundary inside a buffer of CANARY words; the view holds ``data``
    (an input) or FILL (an output)"""

    def __init__(self, n, off=0, data=None):
        self.n, self.lead = int(n), PAD + off
        host = np.full(self.lead + self.n + PAD, CANARY, dtype=np.uint32)
        host[self.lead:self.lead + self.n] = FILL if data is None else np.ascontiguousarray(data, np.float32).reshape(-1).view(np.uint32)
        self.buf = torch.from_numpy(host.view(np.int32)).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.addr = self.buf.data_ptr() + 4 * self.lead

    def ptr(self):
        return ctypes.c_void_p(self.addr)

    def words(self):
        return self.buf.cpu().numpy().view(np.uint32)

    def read(self, shape):
        """the view as float32 -- after checking the canaries either side"""
        w = self.words()
        assert (w[:self.lead] == CANARY).all() and (w[self.lead + self.n:] == CANARY).all(), 'a word beside the output was written'
        return w[self.lead:self.lead + self.n].view(np.float32).reshape(shape)

    def untouched(self):
        w = self.words()
        return bool((w[:self.lead] == CANARY).all() and (w[self.lead + self.n:] == CANARY).all()
                    and (w[self.lead:self.lead + self.n] == FILL).all())


class Launch(object):
    """the device buffers of one case.  Source landmarks of augmentation a sit ``offsets[0] + a`` floats past a 16-byte boundary,
    ``out_kpts`` ``offsets[1]``; boxes and scores 1 and 3 floats past one (4-byte aligned only)."""

    def __init__(self, c):
        self.c = c
        src, out = c.offsets
        self.inputs = [(Block(g.boxes.size, 1, g.boxes), Block(g.scores.size, 3, g.scores), Block(g.kpts.size, (src + a) % 4, g.kpts))
                       for a, g in enumerate(c.segs)]
        self.perm = torch.from_numpy(c.perm).cuda() if c.perm is not None else None
        self.out_b, self.out_s, self.out_k = Block(c.T * 4, 1), Block(c.T * c.S, 3), Block(c.T * c.K * 3, out)
        self.segs = (_lib.AugSegment * max(len(c.segs), 17))()
        for a, (g, (b, s, k)) in enumerate(zip(c.segs, self.inputs)):
            self.segs[a] = _lib.AugSegment(b.addr, s.addr, k.addr, g.n, g.w, g.s, 1 if g.flip else 0)

    def run(self, A=None, S=None, K=None, null=()):
        c = self.c
        p = lambda name, blk: ctypes.c_void_p(0) if name in null else blk.ptr()
        rc = _lib.lib().kgdet_aug_merge(self.segs, i32(len(c.segs) if A is None else A), i32(c.S if S is None else S),
                                        i32(c.K if K is None else K), _lib.ptr(None if 'perm' in null else self.perm),
                                        p('out_boxes', self.out_b), p('out_scores', self.out_s), p('out_kpts', self.out_k),
                                        _lib.current_stream())
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        c = self.c
        return self.out_b.read((c.T, 4)), self.out_s.read((c.T, c.S)), self.out_k.read((c.T, c.K, 3))


def _run(c):
    launch = Launch(c)
    rc = launch.run()
    assert rc == _lib.KGDET_OK, _lib.lib().kgdet_last_error()
    return launch.outputs()


_ref = {}


def _reference(name):
    if name not in _ref:
        c = M.case(name)
        _ref[name] = (c, M.reference_f32(c), M.reference_f64(c))
    return _ref[name]


@pytest.mark.parametrize('name', M.NAMES)
def test_kernel_gives_the_bits_of_the_float32_statement(name):
    c, (b32, s32, k32), (b64, k64, bb, bk) = _reference(name)
    first = _run(c)
    second = _run(c)
    for what, got, again, want in zip(('boxes', 'scores', 'landmarks'), first, second, (b32, s32, k32)):
        assert not (got.view(np.uint32) == FILL).any(), '%s: an element was not written' % what
        assert M.same_bits(got, want), '%s: %s' % (what, M.first_difference(got, want))
        assert M.same_bits(got, again), '%s: two launches differ, %s' % (what, M.first_difference(got, again))
    rb, _ = M.bound_ratio(first[0], b64, bb, name + ' boxes (GPU)')
    rk, _ = M.bound_ratio(first[2], k64, bk, name + ' landmarks (GPU)')
    assert rb <= 1.0 and rk <= 1.0


def test_every_augmentation_empty_writes_nothing():
    c = M.case('K21')
    launch = Launch(c)                                    # (buffers with room: a kernel that ran anyway would show)
    for a in range(len(c.segs)):
        launch.segs[a].n = 0
    assert launch.run() == _lib.KGDET_OK
    assert launch.out_b.untouched() and launch.out_s.untouched() and launch.out_k.untouched()
    assert launch.run(null=('out_boxes', 'out_scores', 'out_kpts', 'perm')) == _lib.KGDET_OK       # T = 0: NULL outputs are fine
    for a in range(len(c.segs)):                          # ... and NULL sources
        launch.segs[a].boxes = launch.segs[a].scores = launch.segs[a].kpts = None
    assert launch.run(null=('out_boxes', 'out_scores', 'out_kpts', 'perm')) == _lib.KGDET_OK
    assert launch.out_b.untouched() and launch.out_s.untouched() and launch.out_k.untouched()


@pytest.mark.parametrize('name,how,status', M.REFUSALS, ids=[r[0] for r in M.REFUSALS])
def test_refusals_leave_the_outputs_untouched(name, how, status):
    c = M.case('K21')
    assert c.segs[0].flip and c.segs[0].n > 0
    launch = Launch(c)
    kw, null = {}, ()
    if 'A' in how:
        kw['A'] = how['A']
        for a in range(len(c.segs), 17):                  # (17 valid segments: only their number is wrong)
            launch.segs[a] = launch.segs[0]
    for key in ('K', 'S'):
        if key in how:
            kw[key] = how[key]
    if 'n' in how:
        launch.segs[1].n = how['n']
    if 'scale' in how:
        launch.segs[1].scale = how['scale']
    if how.get('null') in ('boxes', 'scores', 'kpts'):
        setattr(launch.segs[1], how['null'], None)
    elif 'null' in how:
        null = (how['null'], )
    rc = launch.run(null=null, **kw)
    assert rc == status, (rc, _lib.lib().kgdet_last_error())
    assert _lib.lib().kgdet_last_error()
    assert launch.out_b.untouched() and launch.out_s.untouched() and launch.out_k.untouched()
    with pytest.raises(NotImplementedError if status == _lib.KGDET_E_UNSUPPORTED else RuntimeError):
        _lib.check(rc, 'kgdet_aug_merge')


# --- the wrapper ----------------------------------------------------------------------------------------------------------------
def _metas(c):
    fi = M.flip_indices_of(c.perm)
    return [dict(img_shape=(800, g.w, 3), scale_factor=g.s, flip=g.flip, flip_indices=fi) for g in c.segs]


def _check_wrapper(c, got):
    want = M.reference_f32(c)
    for what, g, w in zip(('boxes', 'scores', 'landmarks'), got, want):
        g = g.cpu().numpy()
        assert g.shape == w.shape, what
        assert M.same_bits(g, w), '%s: %s' % (what, M.first_difference(g, w))


@pytest.mark.parametrize('name', ['rows_K5', 'scales_w999_K5', 'K294'])
def test_wrapper_on_row_slices_of_larger_tensors(name):
    """``k[1:]`` of a contiguous tensor is contiguous, and for K = 5 starts 60 bytes in: 12 past a 16-byte boundary"""
    from kgdet_amd.postprocess import aug_merge_kp
    c = M.case(name)
    lead = [1 + a % 3 for a in range(len(c.segs))]
    bs, ss, ks = [], [], []
    for g, l in zip(c.segs, lead):
        pad = lambda x: torch.from_numpy(np.concatenate([np.full((l, ) + x.shape[1:], 7.25, np.float32), x])).cuda()
        b, s, k = pad(g.boxes)[l:], pad(g.scores)[l:], pad(g.kpts)[l:]
        assert k.is_contiguous() and k.data_ptr() == k.contiguous().data_ptr()
        bs.append(b); ss.append(s); ks.append(k)
    if c.K == 5:
        assert {k.data_ptr() % 16 for k in ks if k.shape[0]} >= {4, 12}
    _check_wrapper(c, aug_merge_kp(bs, ss, ks, _metas(c)))


def test_wrapper_takes_flat_landmarks():
    from kgdet_amd.postprocess import aug_merge_kp
    c = M.case('rows_K5')
    got = aug_merge_kp([torch.from_numpy(g.boxes).cuda() for g in c.segs], [torch.from_numpy(g.scores).cuda() for g in c.segs],
                       [torch.from_numpy(g.kpts.reshape(g.n, 3 * c.K)).cuda() for g in c.segs], _metas(c))
    assert got[2].shape == (c.T, c.K, 3)
    _check_wrapper(c, got)


def test_wrapper_with_no_candidate_at_all():
    from kgdet_amd.postprocess import aug_merge_kp
    c = M.case('K21')
    for g in c.segs:
        g.n, g.boxes, g.scores, g.kpts = 0, g.boxes[:0], g.scores[:0], g.kpts[:0]
    got = aug_merge_kp([torch.from_numpy(g.boxes).cuda() for g in c.segs], [torch.from_numpy(g.scores).cuda() for g in c.segs],
                       [torch.from_numpy(g.kpts).cuda() for g in c.segs], _metas(c))
    assert got[0].shape == (0, 4) and got[1].shape == (0, c.S) and got[2].shape == (0, c.K, 3)
    assert all(t.is_cuda and t.dtype == torch.float32 for t in got)
