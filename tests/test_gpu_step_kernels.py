"""The small kernels that produce the loss value and apply the weight update -- csrc/optim.hip, smooth_l1.hip, focal.hip,
group_norm.hip -- through the C ABI (ctypes, not the Python wrappers: those filter out the argument combinations of interest)
against the float64 references of tests/step_refs.py, at the sizes, alignments and values where such kernels go wrong.

Bars: a bound counted from the fp32 roundings of the kernel's own expression (U = 2^-24 per rounding; derivations at the
assertions and in step_refs.clip_adam_bounds), or the project's 1e-5 of the output scale (focal loss, tests/test_gpu_ops.py).
Outputs whose exact element count matters sit inside a larger buffer of a canary value that must stay untouched.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import step_refs as R

pytestmark = pytest.mark.gpu

U = R.U
CANARY = 12345.678
c_f, c_d, c_i32, c_i64 = ctypes.c_float, ctypes.c_double, ctypes.c_int32, ctypes.c_int64


def _L():
    from kgdet_amd import _lib
    return _lib, _lib.lib()


def _ptr(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * offset) if t is not None else ctypes.c_void_p(0)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _bit_equal(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _ratio(got, want, bound, name, skip=None):
    """max |got - want| / bound (0 / 0 counts as 0), printed before it is asserted"""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(all='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    if skip is not None:
        r = np.where(skip, 0.0, r)
    r = float(np.max(r)) if r.size else 0.0
    print('%s: error %.3f of its bound' % (name, r))
    return r


class Guarded(object):
    """``n`` floats at ``lead`` floats into a buffer of CANARY (lead a multiple of 4: the payload keeps 16-byte alignment)"""

    def __init__(self, n, lead=64, tail=64, fill=None):
        self.n, self.lead = n, lead
        self.buf = torch.full((lead + n + tail,), CANARY, dtype=torch.float32, device='cuda')
        if fill is not None:
            self.view().copy_(torch.as_tensor(fill, dtype=torch.float32).reshape(-1))

    def view(self):
        return self.buf[self.lead:self.lead + self.n]

    def ptr(self):
        return _ptr(self.buf, self.lead)

    def intact(self):
        return bool((self.buf[:self.lead] == CANARY).all()) and bool((self.buf[self.lead + self.n:] == CANARY).all())


# ============================================================================================ optimizer tables
class Table(object):
    """Tensors of the given sizes as slices of four flat buffers (param, grad, exp_avg, exp_avg_sq) of CANARY, the pointer
    table of include/kgdet_hip.h over them: {param, grad, exp_avg, exp_avg_sq, numel, first block}, first block = the blocks of
    kgdet_optim_chunk() elements the rows before take.  ``shift[i]`` floats past a 16-byte boundary for row i (default 0);
    rows listed in ``leave_out`` get their slices but no table row."""

    def __init__(self, sizes, shift=None, leave_out=(), seed=0, lo=-6, hi=3):
        lib, L = _L()
        self.chunk = L.kgdet_optim_chunk()
        shift = shift or {}
        self.offs, at = [], 8
        for i, n in enumerate(sizes):
            at = (at + 3) // 4 * 4 + shift.get(i, 0)
            self.offs.append(at)
            at += n + 8
        self.sizes, self.total = list(sizes), at + 8
        self.rows = [i for i in range(len(sizes)) if i not in leave_out]
        rng = np.random.default_rng(seed)
        host = {k: np.full(self.total, CANARY, np.float32) for k in 'pgmv'}
        self.inside = np.zeros(self.total, bool)
        for i, (o, n) in enumerate(zip(self.offs, sizes)):
            scale = 10.0 ** rng.uniform(lo, hi, n)                    # values from 1e-6 to 1e3 within every tensor
            host['g'][o:o + n] = rng.normal(size=n) * scale
            host['p'][o:o + n] = rng.normal(size=n)
            host['m'][o:o + n] = rng.normal(size=n) * 10.0 ** rng.uniform(lo, 1, n)
            host['v'][o:o + n] = rng.random(n) * 10.0 ** rng.uniform(2 * lo, 2, n)
            if i in self.rows:
                self.inside[o:o + n] = True
        self.host = host
        self.dev = {k: torch.from_numpy(a).cuda() for k, a in host.items()}
        first, rows = 0, []
        for i in self.rows:
            o, n = self.offs[i], sizes[i]
            rows.append([self.dev[k].data_ptr() + 4 * o for k in 'pgmv'] + [n, first])
            first += (n + self.chunk - 1) // self.chunk
        self.blocks = first
        self.table = torch.tensor(rows, dtype=torch.int64).cuda()
        self.partial = Guarded(first)
        self.norm = Guarded(1)

    def upload(self):
        for k in 'pgmv':
            self.dev[k].copy_(torch.from_numpy(self.host[k]))

    def args(self):
        return ctypes.c_void_p(self.table.data_ptr()), c_i32(len(self.rows)), c_i64(self.blocks)

    def grad_norm(self):
        lib, L = _L()
        lib.check(L.kgdet_multi_grad_norm(*self.args(), self.partial.ptr(), self.norm.ptr(), lib.current_stream()), 'multi_grad_norm')
        return self.norm.view().clone()

    def clip_adam(self, norm, max_norm, lr, beta1, beta2, eps, wd, bc1, bc2s):
        lib, L = _L()
        lib.check(L.kgdet_multi_clip_adam(*self.args(), _ptr(norm), c_f(max_norm), c_f(lr), c_d(beta1), c_d(beta2), c_f(eps), c_f(wd),
                                          c_f(bc1), c_f(bc2s), lib.current_stream()), 'multi_clip_adam')

    def clip_adam_dev(self, norm, max_norm, sched, ring, nring, beta1, beta2, eps, wd):
        lib, L = _L()
        lib.check(L.kgdet_multi_clip_adam_dev(*self.args(), _ptr(norm), c_f(max_norm), _ptr(sched),
                                              ctypes.c_void_p(ring.data_ptr()) if ring is not None else ctypes.c_void_p(0), c_i32(nring),
                                              c_d(beta1), c_d(beta2), c_f(eps), c_f(wd), lib.current_stream()), 'multi_clip_adam_dev')

    def read(self):
        return {k: self.dev[k].cpu().numpy() for k in 'pgmv'}


SPECIAL_SIZES = [1, 3, 255, 4095, 4096, 4097, 3 * 4096 + 5]


def _sizes(big, n_rows=304, seed=1):
    rng = np.random.default_rng(seed)
    sizes = list(SPECIAL_SIZES) + [big] + [1, 2, 3, 5, 4096, 4097]          # rows 8..13: the unaligned ones and their neighbours
    sizes += [int(s) for s in rng.integers(1, 3000, n_rows - len(sizes))]
    shift = {8: 1, 9: 2, 10: 3, 11: 1, 12: 2, 13: 3, 20: 1, 40: 2, 60: 3}
    return sizes, shift


def test_grad_norm_over_a_full_size_table():
    """304 rows -- the binary search of opt_row over a table the size of the real one --, a 5.3 M element tensor (1300 blocks:
    the finish kernel's loop strides), every tail length around a block, gradients 1, 2 and 3 floats past a 16-byte boundary
    (the scalar path of multi_sqnorm)."""
    sizes, shift = _sizes(5 * 1024 * 1024 + 77777)
    tb = Table(sizes, shift, seed=2)
    assert len(tb.rows) >= 300 and tb.blocks > 1024
    assert all((tb.dev['g'].data_ptr() + 4 * tb.offs[i]) % 16 == 4 * s for i, s in shift.items())
    got = tb.grad_norm()
    want = R.grad_norm([tb.host['g'][o:o + n] for o, n in zip(tb.offs, tb.sizes)])
    # L = the longest chain of fp32 additions one value passes through: 16 in the thread, 6 shuffle steps, 3 in opt_block_sum,
    # then ceil(total_blocks / 1024) + 6 + 16 in the finish kernel.  All terms are squares (>= 0): the summation tree's bound is
    # L * U relative, + 1 for the square itself and + 1 for the root's own rounding; the root halves it.
    chain = 16 + 6 + 3 + (tb.blocks + 1023) // 1024 + 6 + 16
    rel = abs(float(got) - want) / want
    print('norm %.9g, float64 %.9g: relative error %.3e, bound %.3e' % (float(got), want, rel, (chain + 2) * U / 2))
    assert rel <= (chain + 2) * U / 2
    assert tb.partial.intact() and tb.norm.intact()
    assert _bit_equal(tb.grad_norm(), got)
    assert (tb.dev['g'].cpu().numpy().view(np.int32) == tb.host['g'].view(np.int32)).all()


def _adam_table():
    sizes, shift = _sizes(20000 + 3)
    sizes.append(777)                        # a parameter with slices but no table row: must stay as it is
    tb = Table(sizes, shift, leave_out=(len(sizes) - 1,), seed=3, hi=-1.5)      # ||g|| ~ 4: max_norm 35 leaves it, 0.05 clips
    zero = slice(tb.offs[7] + 100, tb.offs[7] + 400)           # g == m == v == 0 inside the large tensor
    for k in 'gmv':
        tb.host[k][zero] = 0
    tb.m0, tb.g0 = slice(tb.offs[7] + 1000, tb.offs[7] + 1600), slice(tb.offs[7] + 2000, tb.offs[7] + 2600)
    tb.host['m'][tb.m0] = 0                  # exp_avg == 0, and grad == 0: where each form of the lerp is ONE rounding
    tb.host['g'][tb.g0] = 0
    return tb, zero


def _check_step(tb, before, after, norm, max_norm, lr, beta1, beta2, eps, wd, t, tag=''):
    sel = tb.inside
    ref = R.clip_adam_step(*(before[k][sel] for k in 'pgmv'), norm, max_norm, lr, beta1, beta2, eps, wd, t)
    bg, bm, bv, bp = R.clip_adam_bounds(*(before[k][sel] for k in 'pgmv'), norm, max_norm, lr, beta1, beta2, eps, wd, t)
    for k in 'pgmv':      # everything outside the table's tensors: canaries, and the parameter that has no row
        assert (after[k][~sel].view(np.int32) == before[k][~sel].view(np.int32)).all(), k
    scaled = not R.clip_coef(norm, max_norm) >= 1.0
    if not scaled:
        assert (after['g'].view(np.int32) == before['g'].view(np.int32)).all()
    # k of each output (step_refs.clip_adam_bounds): g 3 when scaled; m k_g + (2 with weight decay) + 4, or + 5 in the
    # w1 >= 0.5 form; v 2 (k_g + (2)) + 6; p (k_m + 1) + (k_v + 1) / 2 + 8 -- bound (k + 1) U of the magnitudes entering the last
    # addition: |g'|; max(|m|, |g'| + |p wd|); beta2 v + (1 - beta2) (|g'| + |p wd|)^2; |p| + |step|.
    # The float32 restatement of the expression measures at most 0.5 / 0.3 / 0.5 / 1.0 of these bounds (tests/test_step_refs.py).
    for k, want, bound in (('g', ref[1], bg), ('m', ref[2], bm), ('v', ref[3], bv), ('p', ref[0], bp)):
        assert _ratio(after[k][sel], want, bound, tag + k) <= 1.0, k
    return ref


@pytest.mark.parametrize('t', [1, 2, 1000])
@pytest.mark.parametrize('max_norm', [35.0, 0.05, 0.0])              # inactive, active, no clipping and norm = NULL
@pytest.mark.parametrize('beta1', [0.9, 0.3])                        # both lerp forms of optim.hip:121
@pytest.mark.parametrize('wd', [0.0, 1e-4])
def test_clip_adam_one_step(wd, beta1, max_norm, t):
    tb, zero = _adam_table()
    tb.upload()
    f = np.float32
    beta2, lr, eps, wd = 0.999, float(f(1e-3)), float(f(1e-8)), float(f(wd))
    norm_dev, norm = None, None
    if max_norm > 0:
        norm_dev = tb.grad_norm()
        norm = float(norm_dev)
        assert (R.clip_coef(norm, max_norm) < 1.0) == (max_norm < 1.0)
    before = tb.read()
    bc1, bc2s = float(f(1.0 - beta1 ** t)), float(f(math.sqrt(1.0 - beta2 ** t)))
    tb.clip_adam(norm_dev, max_norm, lr, beta1, beta2, eps, wd, bc1, bc2s)
    after = tb.read()
    _check_step(tb, before, after, norm, max_norm, lr, beta1, beta2, eps, wd, t)
    if wd == 0 and max_norm != 0.05:
        # lerp(exp_avg, grad, w1) in torch's two forms (optim.hip:121): exp_avg + w1 (grad - exp_avg) for w1 < 0.5 is exactly
        # fl(w1 grad) at exp_avg == 0; grad - (grad - exp_avg) (1 - w1) otherwise is exactly fl(exp_avg fl(1 - w1)) at grad == 0
        # (with or without a fused multiply-add).  The other form in either place rounds twice more and differs in many elements.
        w1 = f(1.0 - beta1)
        if w1 < 0.5:
            assert (after['m'][tb.m0] == w1 * before['g'][tb.m0]).all()
        else:
            assert (after['m'][tb.g0] == before['m'][tb.g0] * (f(1.0) - w1)).all()
    if wd == 0:      # nothing to move: the parameter keeps its bits
        assert (after['p'][zero].view(np.int32) == before['p'][zero].view(np.int32)).all()
        assert (after['m'][zero] == 0).all() and (after['v'][zero] == 0).all()


def test_clip_adam_steps_from_the_reference_state():
    """five consecutive steps, each from the float64 reference's state rounded to fp32: the per-step bar stays the one-step bar"""
    tb, _ = _adam_table()
    f = np.float32
    beta1, beta2, lr, eps, wd = 0.9, 0.999, float(f(1e-3)), float(f(1e-8)), float(f(1e-4))
    rng = np.random.default_rng(11)
    for t in range(1, 6):
        sel = tb.inside
        tb.host['g'][sel] = (rng.normal(size=int(sel.sum())) * 10.0 ** rng.uniform(-6, -1.5, int(sel.sum()))).astype(f)
        tb.upload()
        norm_dev = tb.grad_norm()
        before = tb.read()
        tb.clip_adam(norm_dev, 35.0 if t % 2 else 0.05, lr, beta1, beta2, eps, wd, float(f(1.0 - beta1 ** t)), float(f(math.sqrt(1.0 - beta2 ** t))))
        ref = _check_step(tb, before, tb.read(), float(norm_dev), 35.0 if t % 2 else 0.05, lr, beta1, beta2, eps, wd, t, 'step %d ' % t)
        for k, a in zip('pmv', (ref[0], ref[2], ref[3])):
            tb.host[k][sel] = a.astype(f)


def test_clip_boundary_just_above_and_just_below_one():
    """two norms for which max_norm / (norm + 1e-6), evaluated in fp32 as the kernel does, is the float just above 1 and the
    float just below 1: gradients bit-unchanged, and every gradient equal to fl(g * coef)"""
    f = np.float32
    tb, _ = _adam_table()
    max_norm = f(31.0)      # at the upper end of its binade the quotient can land one float below 1; 35 / norm steps over it

    def coef_of(norm):
        return max_norm / (f(norm) + f(1e-6))
    found = {}
    norm = max_norm
    for _ in range(64):
        norm = np.nextafter(norm, f(0))
    for _ in range(128):
        c = coef_of(norm)
        if c == np.nextafter(f(1), f(2)):
            found['above'] = norm
        if c == np.nextafter(f(1), f(0)):
            found['below'] = norm
        norm = np.nextafter(norm, f(100))
    assert set(found) == {'above', 'below'}, found
    for which, norm in found.items():
        tb.upload()
        before = tb.read()
        norm_dev = torch.tensor([float(norm)], dtype=torch.float32, device='cuda')
        tb.clip_adam(norm_dev, float(max_norm), 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.0316)
        after = tb.read()
        if which == 'above':
            assert (after['g'].view(np.int32) == before['g'].view(np.int32)).all()
        else:
            want = np.where(tb.inside, before['g'] * coef_of(norm), before['g']).astype(f)
            assert (after['g'].view(np.int32) == want.view(np.int32)).all()
            assert (after['g'][tb.inside] != before['g'][tb.inside]).any()


# ============================================================================================ device schedule
def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize('t0', [0, 1000])
def test_device_schedule_over_two_wraps_of_the_ring(t0):
    """130 consecutive calls of kgdet_multi_clip_adam_dev (the schedule of the graphed step) over a 64-slot page-locked ring,
    from a fresh schedule and from a resumed one: after every call the step count, this step's learning rate (bit-equal), the
    two bias corrections (1 ulp: the device's pow against the host's libm), and parameters and moments bit-equal to
    kgdet_multi_clip_adam on a copy of the state with the schedule's values as arguments."""
    f = np.float32
    sizes = [1, 3, 255, 4097, 700, 64]
    A, B = Table(sizes, {1: 1, 4: 3}, seed=5, lo=-3, hi=1), Table(sizes, {1: 1, 4: 3}, seed=5, lo=-3, hi=1)
    beta1, beta2, eps, wd, base, ring_n = 0.9, 0.999, 1e-8, 1e-4, 1e-3, 64
    ring = torch.full((ring_n,), 7.0, dtype=torch.float32).pin_memory()
    sched = Guarded(4, fill=[0.5, -1.0, -1.0, float(t0)])
    norm = torch.tensor([30.0], dtype=torch.float32, device='cuda')
    pool = [torch.from_numpy(np.where(A.inside, np.random.default_rng(k).normal(size=A.total) * 3, CANARY).astype(f)).cuda() for k in range(4)]
    for k in range(1, 131):
        s = t0 + k
        lr = f(base * (1 + s / 1000.0))
        ring[s % ring_n] = float(lr)
        for T in (A, B):
            T.dev['g'].copy_(pool[k % 4])
        for key in 'pmv':
            B.dev[key].copy_(A.dev[key])
        A.clip_adam_dev(norm, 0.5, sched.view(), ring, ring_n, beta1, beta2, eps, wd)
        torch.cuda.synchronize()
        sc = sched.view().cpu().numpy()
        assert sc[3] == s, (k, sc)
        assert sc[0].view(np.int32) == lr.view(np.int32), (k, sc, lr)
        assert _ulps(sc[1], f(1.0 - beta1 ** s)) <= 1, (k, sc)
        assert _ulps(sc[2], f(math.sqrt(1.0 - beta2 ** s))) <= 1, (k, sc)
        B.clip_adam(norm, 0.5, float(sc[0]), beta1, beta2, eps, wd, float(sc[1]), float(sc[2]))
        for key in 'pgmv':
            assert _bit_equal(A.dev[key], B.dev[key]), (k, key)
    assert sched.intact()
    assert not _bit_equal(A.dev['g'], pool[130 % 4])           # (the clip was active)
    A.clip_adam_dev(norm, 0.5, sched.view(), None, 0, beta1, beta2, eps, wd)      # no ring: the learning rate stays
    sc2 = sched.view().cpu().numpy()
    assert sc2[3] == t0 + 131 and sc2[0].view(np.int32) == sc[0].view(np.int32)


# ============================================================================================ non-finite gradients
@pytest.mark.parametrize('route', ['args', 'device_schedule'])
@pytest.mark.parametrize('bad', ['nan', 'inf'])
def test_non_finite_gradient_follows_clip_grad_norm_and_adam(bad, route):
    """What torch does (include/kgdet_hip.h, kgdet_multi_clip_adam): clip_grad_norm_ multiplies every gradient by the clamped
    coefficient.  A NaN among the gradients makes the norm and the coefficient NaN: every gradient, moment and parameter of
    the table becomes NaN.  An infinite one makes the coefficient 0: that element becomes NaN (inf * 0), every other gradient
    0, and the step goes on from the moments alone."""
    f = np.float32
    tb = Table([5, 4097, 300], {2: 1}, seed=9, lo=-2, hi=1)
    at = tb.offs[1] + 4000
    tb.host['g'][at] = f(bad)
    tb.upload()
    norm_dev = tb.grad_norm()
    assert math.isnan(float(norm_dev)) if bad == 'nan' else math.isinf(float(norm_dev))
    before = tb.read()
    beta1, beta2, lr, eps, t = 0.9, 0.999, float(f(1e-3)), float(f(1e-8)), 3
    bc1, bc2s = f(1.0 - beta1 ** t), f(math.sqrt(1.0 - beta2 ** t))
    if route == 'args':
        tb.clip_adam(norm_dev, 35.0, lr, beta1, beta2, eps, 0.0, float(bc1), float(bc2s))
    else:
        sched = torch.tensor([lr, 0, 0, t - 1], dtype=torch.float32, device='cuda')
        tb.clip_adam_dev(norm_dev, 35.0, sched, None, 0, beta1, beta2, eps, 0.0)
    after = tb.read()
    sel = tb.inside
    assert not np.isfinite(after['p'][at])
    for k in 'pgmv':
        assert (after[k][~sel].view(np.int32) == before[k][~sel].view(np.int32)).all(), k
    if bad == 'nan':
        for k in 'pgmv':
            assert np.isnan(after[k][sel]).all(), k
    else:
        others = sel.copy()
        others[at] = False
        assert (after['g'][others] == 0).all() and np.isnan(after['g'][at]) and np.isnan(after['p'][at])
        zero_g = np.where(others, 0, before['g']).astype(f)
        ref = R.clip_adam_step(before['p'][others], zero_g[others], before['m'][others], before['v'][others], None, 0.0, lr, beta1,
                               beta2, eps, 0.0, t)
        bounds = R.clip_adam_bounds(before['p'][others], zero_g[others], before['m'][others], before['v'][others], None, 0.0, lr,
                                    beta1, beta2, eps, 0.0, t)
        for k, want, bound in (('m', ref[2], bounds[1]), ('v', ref[3], bounds[2]), ('p', ref[0], bounds[3])):
            assert np.isfinite(after[k][others]).all()
            assert _ratio(after[k][others], want, bound, k) <= 1.0, k


# ============================================================================================ smooth L1
def _sl1_forward(pred, target, weight, n, beta, divisor):
    lib, L = _L()
    partial, out = Guarded(L.kgdet_smooth_l1_partials()), Guarded(1)
    lib.check(L.kgdet_smooth_l1_sum_forward(_ptr(pred), _ptr(target), _ptr(weight), c_i64(n), c_f(beta), c_f(divisor), partial.ptr(),
                                            out.ptr(), lib.current_stream()), 'smooth_l1_sum_forward')
    assert partial.intact() and out.intact()
    return out.view().clone()


def _sl1_backward(pred, target, weight, gsum, n, beta, divisor):
    lib, L = _L()
    grad = Guarded(n)
    lib.check(L.kgdet_smooth_l1_sum_backward(_ptr(pred), _ptr(target), _ptr(weight), _ptr(gsum), c_i64(n), c_f(beta), c_f(divisor),
                                             grad.ptr(), lib.current_stream()), 'smooth_l1_sum_backward')
    assert grad.intact()
    return grad.view().clone()


def _sl1_check(pred, target, weight, beta, divisor, g=0.37, cap=None, tag=''):
    """forward and backward of one case (host float32 arrays; weight may be None) against float64"""
    f = np.float32
    n = pred.size
    beta_f, g_f = float(f(beta)), float(f(g))
    dp, dt = torch.from_numpy(pred.reshape(-1)).cuda(), torch.from_numpy(target.reshape(-1)).cuda()
    dw = None if weight is None else torch.from_numpy(weight.reshape(-1)).cuda()
    gsum = torch.tensor([g_f], dtype=torch.float32, device='cuda')
    got = _sl1_forward(dp, dt, dw, n, beta_f, divisor)
    grad = _sl1_backward(dp, dt, dw, gsum, n, beta_f, divisor)
    assert _bit_equal(_sl1_forward(dp, dt, dw, n, beta_f, divisor), got)
    assert _bit_equal(_sl1_backward(dp, dt, dw, gsum, n, beta_f, divisor), grad)
    got, grad = float(got), grad.cpu().numpy()
    # the float64 side only over the elements that weigh: the rest contribute exactly 0 to both
    flat = lambda a: None if a is None else a.reshape(-1)
    sel = np.ones(n, bool) if weight is None else flat(weight) != 0
    p, t = flat(pred)[sel], flat(target)[sel]
    w = np.ones(int(sel.sum())) if weight is None else flat(weight)[sel].astype(np.float64)
    x, l = R.smooth_l1_terms(p, t, beta_f, divisor)
    want = float(np.sum(w * l))
    # forward bar: the cancellation of p / d - t / d -- two quotients rounded at |p| / |d| and |t| / |d|, l' <= 1 -- plus the
    # summation chain: ceil(n / 65536) additions in the thread (256 workgroups of 256), 6 shuffle steps and 3 additions per
    # block sum, the same 9 again in the finish kernel; + 2 for the roundings of l itself and of l * w
    chain = (n + 65535) // 65536 + 9 + 9
    bound = float(np.sum(w * (np.abs(p) + np.abs(t)))) / abs(divisor) * 2.0 ** -23 + (chain + 2) * U * want
    print('%ssum %.9g, float64 %.9g: error %.3e, bound %.3e' % (tag, got, want, abs(got - want), bound))
    assert abs(got - want) <= bound
    assert (grad[~sel] == 0).all()
    ref = R.smooth_l1_grad(p, t, w, g_f, beta_f, divisor)
    window = R.smooth_l1_branch_window(p, t, beta_f, divisor)
    if cap is not None:      # the reference alone decides who is left out, and it may be few
        assert window.sum() <= cap * sel.sum(), (int(window.sum()), int(sel.sum()))
    # backward bar: g * w, * l', / d and (quadratic branch) x / beta: 4 roundings of the result; on the quadratic branch the
    # roundings of the two quotients and of their difference, carried through / beta * g w / d.  (float32 restatement: at most
    # 0.6 of it, tests/test_step_refs.py)
    bound = 4 * U * np.abs(ref) + np.where(np.abs(x) < beta_f, (np.abs(p) + np.abs(t)) / abs(divisor) * 2.0 ** -23 / beta_f
                                           * np.abs(g_f * w / divisor), 0.0)
    assert _ratio(grad[sel], ref, bound, tag + 'grad_pred', skip=window) <= 1.0
    assert ((grad[sel] == 0) == (ref == 0))[~window].all()
    return got, grad


def test_smooth_l1_dense_targets_and_non_finite_predictions_under_zero_weight():
    """[33600, 588] with 12 positive rows and a few single elements (19.7 M elements: both grid-stride loops take many trips with
    a ragged last one), then the same with inf / NaN predictions where whole waves weigh zero: the documented difference from
    the reference -- the sum stays finite and equal, the gradient exactly 0 there."""
    pred, target, weight = R.dense_smooth_l1_inputs()
    got, grad = _sl1_check(pred, target, weight, 1.0 / 9.0, 128.0, cap=1e-3, tag='dense ')
    zero = R.zero_weight_waves(weight).reshape(pred.shape)
    rows = np.flatnonzero(zero.all(1))
    assert rows.size > 30000
    bad = pred.copy()
    bad[rows[::7]] = np.inf
    bad[rows[3::7]] = np.nan
    bad[rows[5::7], ::2] = -np.inf
    assert not np.isfinite(bad[zero]).all() and np.isfinite(bad[~zero]).all()
    got2, grad2 = _sl1_check(bad, target, weight, 1.0 / 9.0, 128.0, tag='dense, non-finite ')
    assert math.isfinite(got2) and got2 == got
    assert (grad2.view(np.int32) == grad.view(np.int32)).all()


@pytest.mark.parametrize('with_weight', [True, False])
@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 255, 257, 2048 * 256 + 1])
def test_smooth_l1_sizes(n, with_weight):
    rng = np.random.default_rng(n + 1)
    f = np.float32
    pred = (300 + 40 * rng.standard_normal(n)).astype(f)
    target = (pred + 20 * rng.standard_normal(n)).astype(f)
    target[::3] = pred[::3]
    weight = None
    if with_weight:
        weight = ((rng.random(n) > 0.5) * rng.random(n)).astype(f)
        for a in range(64, n, 256):          # every fourth wave weighs zero as a whole; so does a ragged last one
            weight[a:a + 64] = 0
        if n > 64:
            weight[n // 64 * 64:] = 0
    if n == 0:
        lib, L = _L()
        dummy = torch.zeros(4, device='cuda')
        assert float(_sl1_forward(dummy, dummy, dummy if with_weight else None, 0, 0.5, 128.0)) == 0.0
        grad = Guarded(4)
        lib.check(L.kgdet_smooth_l1_sum_backward(_ptr(dummy), _ptr(dummy), None, _ptr(dummy), c_i64(0), c_f(0.5), c_f(128.0), grad.ptr(),
                                                 lib.current_stream()), 'smooth_l1_sum_backward')
        assert (grad.buf == CANARY).all()
        return
    _sl1_check(pred, target, weight, 1.0 / 9.0, 128.0)


def test_smooth_l1_negative_divisor():
    rng = np.random.default_rng(4)
    f = np.float32
    pred = (300 + 40 * rng.standard_normal(70001)).astype(f)
    target = (pred + 5 * rng.standard_normal(70001)).astype(f)
    weight = ((rng.random(70001) > 0.3) * rng.random(70001)).astype(f)
    got, grad = _sl1_check(pred, target, weight, 1.0 / 9.0, -32.0)
    assert got > 0
    sel = (weight != 0) & (np.abs(pred - target) > 32.0 / 9.0 * 1.01)
    # the loss is a function of |x|: the gradient keeps the sign of pred - target whatever the divisor's sign
    assert sel.sum() > 1000 and (np.sign(grad[sel]) == np.sign(pred[sel] - target[sel])).all()


@pytest.mark.parametrize('with_weight', [True, False])
def test_smooth_l1_branch_boundary(with_weight):
    """inputs of powers of two, p / d - t / d exact: |x| == beta is on the linear branch (value beta / 2, gradient +-1), the float
    below beta on the quadratic one (gradient x / beta = 1 - 2^-24, not 1), x == 0 has gradient exactly 0"""
    f = np.float32
    beta, d = f(0.125), f(4.0)
    below = np.nextafter(f(0.5), f(0))                 # / 4: the float below 0.125
    pred = np.array([1.0, 0.5, below, -below, 0.5, 3.0, -0.5, 0.0] * 16, f)
    target = np.array([0.5, 1.0, 0.0, 0.0, 0.5, 3.0, 0.0, 0.5] * 16, f)
    x = pred / d - target / d
    assert (x[:8] == np.array([0.125, -0.125, below / 4, -below / 4, 0, 0, -0.125, -0.125], f)).all()
    weight = np.ones(128, f) if with_weight else None
    dp, dt = torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda()
    dw = None if weight is None else torch.from_numpy(weight).cuda()
    grad = _sl1_backward(dp, dt, dw, torch.ones(1, device='cuda'), 128, float(beta), float(d)).cpu().numpy()
    q = f(1.0) - f(2.0 ** -24)
    want = np.array([1, -1, q, -q, 0, 0, -1, -1] * 16, f) / d
    assert (grad.view(np.int32) == want.view(np.int32)).all(), grad[:8] * d
    total = float(_sl1_forward(dp, dt, dw, 128, float(beta), float(d)))
    lq = 0.5 * float(below / 4) ** 2 / 0.125
    assert abs(total - 16 * (4 * 0.0625 + 2 * lq)) <= 4 * U * total


# ============================================================================================ focal loss
SPECIAL_LOGITS = [0.0, 1e-8, -1e-8, 16.7, -16.7, 30.0, -30.0, 80.0, -80.0, 88.8, -88.8, 104.0, -104.0, 1e4, -1e4]


def _focal_run(logits, target, dl, gamma, alpha):
    lib, L = _L()
    num, C = logits.shape
    x, t, d = torch.from_numpy(logits).cuda(), torch.from_numpy(target).cuda(), torch.from_numpy(dl).cuda()
    out = []
    for _ in range(2):
        loss, grad = Guarded(num * C), Guarded(num * C)
        lib.check(L.kgdet_sigmoid_focal_loss_forward(_ptr(x), ctypes.c_void_p(t.data_ptr()), c_i64(num), c_i32(C), c_f(gamma),
                                                     c_f(alpha), loss.ptr(), lib.current_stream()), 'focal_forward')
        lib.check(L.kgdet_sigmoid_focal_loss_backward(_ptr(x), ctypes.c_void_p(t.data_ptr()), _ptr(d), c_i64(num), c_i32(C),
                                                      c_f(gamma), c_f(alpha), grad.ptr(), lib.current_stream()), 'focal_backward')
        assert loss.intact() and grad.intact()
        out.append((loss.view().clone(), grad.view().clone()))
    assert _bit_equal(out[0][0], out[1][0]) and _bit_equal(out[0][1], out[1][1])
    return out[0][0].cpu().numpy().reshape(num, C), out[0][1].cpu().numpy().reshape(num, C)


def _scaled_err(got, want, mask):
    if not mask.any():
        return 0.0
    return float(np.abs(got - want)[mask].max() / max(np.abs(want[mask]).max(), 1e-6))


def _focal_case(num, C, gamma, alpha, seed=0):
    f = np.float32
    rng = np.random.default_rng(seed)
    logits = (rng.normal(size=(num, C)) * 3).astype(f)
    target = rng.integers(0, C + 1, num)
    target[rng.random(num) < 0.05] = -1          # ignore
    target[rng.random(num) < 0.05] = C + 5       # every class negative
    target[rng.random(num) < 0.02] = C
    n_sp = len(SPECIAL_LOGITS)
    for i, val in enumerate(SPECIAL_LOGITS):     # one planted row per special value as a positive, one as negatives, one ignored
        logits[3 * i:3 * i + 3] = val
        target[3 * i:3 * i + 3] = [1, 0, -1]
    dl = rng.normal(size=(num, C)).astype(f)
    loss, grad = _focal_run(logits, target, dl, gamma, alpha)
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    assert (loss >= 0).all()
    c1, c2 = R._focal_classes(target, C)
    # d loss / d x is <= 0 for the positive class and >= 0 for the negatives
    sign = np.where(c1, -1.0, 1.0) * np.sign(dl)
    assert (grad * sign >= 0).all()
    ignored = target < 0
    assert ignored.sum() >= n_sp and (loss[ignored] == 0).all() and (grad[ignored] == 0).all()
    assert (loss[target == 0] >= 0).all() and (target > C).any()
    # inside |x| <= 80 the project's bar, 1e-5 of the output scale, against float64: over the planted rows (scale ~ 80) and,
    # separately, over the bulk at its own (smaller) scale; beyond 80 the formula saturates in fp32 -- p = 0 ->
    # log(max(p, FLT_MIN)), as in the reference's CUDA code -- and the bar is the float32 restatement of the same expressions
    planted = np.zeros((num, C), bool)
    planted[:3 * n_sp] = True
    inside = np.abs(logits) <= 80
    for name, got, w64, w32 in (('loss', loss, R.focal_forward(logits, target, gamma, alpha), R.focal_forward_f32(logits, target, gamma, alpha)),
                                ('grad', grad, R.focal_backward(logits, target, dl, gamma, alpha),
                                 R.focal_backward_f32(logits, target, dl, gamma, alpha))):
        errs = (_scaled_err(got, w64, inside & ~planted), _scaled_err(got, w64, inside & planted), _scaled_err(got, w32, ~inside))
        print('%s: %.2e (bulk) %.2e (planted, |x| <= 80) %.2e (beyond, against float32) of the output scale' % ((name,) + errs))
        assert max(errs) < 1e-5, (name, errs)


@pytest.mark.parametrize('gamma,alpha', [(2.0, 0.25), (1.5, 0.5), (0.0, 1.0)])
def test_focal_three_trips_of_the_capped_grid(gamma, alpha):
    """120001 x 13 = 1.56 M elements: the launch is capped at 2048 workgroups, so the grid-stride loop takes three trips, the last
    one ragged"""
    _focal_case(120001, 13, gamma, alpha)


@pytest.mark.parametrize('alpha', [0.25, 0.5, 1.0])
@pytest.mark.parametrize('gamma', [0.0, 1.5, 2.0])
@pytest.mark.parametrize('C', [1, 13, 80])
def test_focal_classes_gamma_alpha(C, gamma, alpha):
    _focal_case(2503, C, gamma, alpha, seed=C)


def test_focal_no_rows():
    lib, L = _L()
    loss = Guarded(8)
    x, t = torch.zeros(8, device='cuda'), torch.zeros(8, dtype=torch.int64, device='cuda')
    lib.check(L.kgdet_sigmoid_focal_loss_forward(_ptr(x), ctypes.c_void_p(t.data_ptr()), c_i64(0), c_i32(13), c_f(2.0), c_f(0.25),
                                                 loss.ptr(), lib.current_stream()), 'focal_forward')
    lib.check(L.kgdet_sigmoid_focal_loss_backward(_ptr(x), ctypes.c_void_p(t.data_ptr()), _ptr(x), c_i64(0), c_i32(13), c_f(2.0),
                                                  c_f(0.25), loss.ptr(), lib.current_stream()), 'focal_backward')
    assert (loss.buf == CANARY).all()


# ============================================================================================ GroupNorm (+ ReLU), fp32
GN_EPS = 1e-5


def _gn_data(kind, N, C, G, HW, rng):
    f = np.float32
    if kind == 'mean50':
        x = (50 + 0.05 * rng.standard_normal((N, C, HW))).astype(f)
    else:
        x = (3 * rng.standard_normal((N, C, HW)) + 1).astype(f)
    if kind == 'const':      # the last group of the first image holds one value (2.0: every partial sum of it is exact in fp32)
        x[0, C - C // G:] = 2.0
    return x


def _gn_run(x, gamma, beta, G, relu, gy, want_gx, split):
    """forward + backward through the plain or the _split entry points; every output inside canaries; backward twice"""
    lib, L = _L()
    N, C, HW = x.shape
    dx, dgy = torch.from_numpy(x).cuda(), torch.from_numpy(gy).cuda()
    dg = None if gamma is None else torch.from_numpy(gamma).cuda()
    db = None if beta is None else torch.from_numpy(beta).cuda()
    y, mean, rstd = Guarded(x.size), Guarded(N * G), Guarded(N * G)
    st = lib.current_stream()
    if split:
        L.kgdet_gn_act_scratch_floats.restype = ctypes.c_size_t
        ns = L.kgdet_gn_act_scratch_floats(c_i64(N), c_i32(C), c_i32(G), c_i64(HW))
        scratch = Guarded(max(ns, 1))
        lib.check(L.kgdet_gn_act_forward_split(_ptr(dx), _ptr(dg), _ptr(db), c_i32(G), c_f(GN_EPS), c_i32(relu), y.ptr(), mean.ptr(),
                                               rstd.ptr(), scratch.ptr() if ns else None, c_i64(N), c_i32(C), c_i64(HW), st), 'gn_act_forward_split')
        assert scratch.intact()
    else:
        lib.check(L.kgdet_gn_act_forward(_ptr(dx), _ptr(dg), _ptr(db), c_i32(G), c_f(GN_EPS), c_i32(relu), y.ptr(), mean.ptr(), rstd.ptr(),
                                         c_i64(N), c_i32(C), c_i64(HW), st), 'gn_act_forward')
    assert y.intact() and mean.intact() and rstd.intact()
    outs = []
    for _ in range(2):
        gx, dgb = Guarded(x.size), Guarded(2 * N * C)
        gxp = gx.ptr() if want_gx else None
        if split:
            lib.check(L.kgdet_gn_act_backward_split(_ptr(dgy), _ptr(dx), y.ptr(), _ptr(dg), mean.ptr(), rstd.ptr(), c_i32(G), c_i32(relu),
                                                    gxp, dgb.ptr(), scratch.ptr() if ns else None, c_i64(N), c_i32(C), c_i64(HW), st),
                      'gn_act_backward_split')
            assert scratch.intact()
        else:
            lib.check(L.kgdet_gn_act_backward(_ptr(dgy), _ptr(dx), y.ptr(), _ptr(dg), mean.ptr(), rstd.ptr(), c_i32(G), c_i32(relu), gxp,
                                              dgb.ptr(), c_i64(N), c_i32(C), c_i64(HW), st), 'gn_act_backward')
        assert gx.intact() and dgb.intact()
        if not want_gx:
            assert (gx.buf == CANARY).all()
        outs.append((gx.view().clone(), dgb.view().clone()))
    assert _bit_equal(outs[0][0], outs[1][0]) and _bit_equal(outs[0][1], outs[1][1])      # deterministic
    return dict(y=y.view().cpu().numpy().reshape(x.shape), mean=mean.view().cpu().numpy(), rstd=rstd.view().cpu().numpy(),
                grad_x=outs[0][0].cpu().numpy().reshape(x.shape), dgamma=outs[0][1].cpu().numpy()[:N * C].reshape(N, C),
                dbeta=outs[0][1].cpu().numpy()[N * C:].reshape(N, C))


def _gn_bounds(x, gamma, beta, G, gy, got, ref, relu, slices):
    """fp32 rounding bounds of csrc/group_norm.hip around the float64 reference, from the kernel's expressions (U = 2^-24 per
    rounding; a sum of n terms through a chain of L additions is within L U sum |terms|).  Per (image, group) of n = D HW values:
      mean    Ls U mean|x|,   Ls = ceil(n / 1024) + 6 + 16 + 1 (thread, shuffle, the 16 wave sums, the division); the sliced
              kernels: a slice's n, + S + 2 for the weighted mean of the slice means
      rstd    the centred squares are >= 0: relative (3 + Ls + 2) U / 2 + 2 U (d d has 3 roundings; / n, + eps; sqrt, 1 / .),
              + (err_mean rstd)^2 / 2 (a shifted mean adds n err^2 to the squares; the first-order term sums to zero)
      y       4 U (|x - mean| rstd |gamma| + |beta|)   (the difference, two products, the sum)
              + err_mean rstd |gamma|                  (the rounding of the fp32 mean: what |mean| >> std exercises)
              + rel_rstd |x - mean| rstd |gamma|;  the sliced forward computes x sc + (beta - mean sc): 3 U (|x| + |mean|) rstd |gamma| more
      db_c    Lc U sum|g'|, ds_c: (Lc + 1) U sum|g' x|,  Lc = the chain of a channel's sum (below)
      dgamma  (ds - mean db) rstd, the cancellation explicit: rstd (err_ds + |mean| err_db + |db| err_mean + 2 U (|mean db| + |ds|))
              + (rel_rstd + 2 U) |dgamma|
      grad_x  g' gamma rstd + c2 x + c3,  c2 = (S1 mean - S2) rstd^3 / n,  c3 = -c2 mean - S1 rstd / n:
              the error of c2 (that of S1 mean - S2 as for dgamma, summed over the D channels with D more roundings, 3 rel_rstd and
              4 roundings of its own) times |x - mean|;  3 U |c2| (|x| + |mean|) for the roundings of c2 x, c2 mean and their sum
              (the other cancellation |mean| >> std exercises) + |c2| err_mean;  the error of S1 rstd / n;  (rel_rstd + 4 U) |g' gamma rstd|;
              2 U |grad_x|.
    These are worst-case bounds of sums of HW signed terms: for dgamma, dbeta and the constants of grad_x they are looser than the
    2e-6 of the output scale tests/test_gpu_ops.py uses for 3 randn + 1 data (a random walk of roundings stays far below L U sum|.|;
    measured: at most 0.17 of any bound); y and grad_x of that data are ALSO held to the 2e-6 (_gn_case).
    ``got`` supplies the kernel's ReLU mask; every magnitude is taken from float64 data."""
    N, C, HW = x.shape
    D = C // G
    n = D * HW
    X = x.astype(np.float64).reshape(N, G, D, HW)
    gam = np.ones(C) if gamma is None else gamma.astype(np.float64)
    bet = np.zeros(C) if beta is None else beta.astype(np.float64)
    gam4, bet4 = gam.reshape(1, G, D, 1), bet.reshape(1, G, D, 1)
    mean = ref['mean'].reshape(N, G, 1, 1)
    rstd = ref['rstd'].reshape(N, G, 1, 1)
    if slices > 1:
        per = (HW + slices - 1) // slices
        Ls = (D * per + 1023) // 1024 + 6 + 16 + 1 + slices + 2
    else:
        Ls = (n + 1023) // 1024 + 6 + 16 + 1
    err_mean = Ls * U * np.abs(X).mean((2, 3), keepdims=True)
    rel_rstd = ((3 + Ls + 2 + (2 * slices if slices > 1 else 0)) / 2.0 + 2) * U + (err_mean * rstd) ** 2 / 2
    dev = np.abs(X - mean)
    by = 4 * U * (dev * rstd * np.abs(gam4) + np.abs(bet4)) + err_mean * rstd * np.abs(gam4) + rel_rstd * dev * rstd * np.abs(gam4)
    if slices > 1:
        by = by + 3 * U * (np.abs(X) + np.abs(mean)) * rstd * np.abs(gam4)
    out = dict(y=by.reshape(x.shape), mean=err_mean.reshape(-1), rstd=(rel_rstd * rstd).reshape(-1))
    if gy is None:
        return out
    gp = gy.astype(np.float64).reshape(N, G, D, HW)
    if relu:
        gp = gp * (got['y'].reshape(N, G, D, HW) > 0)
    # the chain of one channel's sums: a lane's share of the pixels, the product, 6 shuffle steps, the wave slices of the channel;
    # sliced: the slices of the pixels on top
    wpc = 16 // D if D <= 16 else 1
    if slices > 1:
        Lc = ((HW + slices - 1) // slices + 64 * wpc - 1) // (64 * wpc) + 1 + 6 + wpc + slices
    else:
        Lc = (HW + 64 * wpc - 1) // (64 * wpc) + 1 + 6 + wpc
    A, B = np.abs(gp * X).sum(3, keepdims=True), np.abs(gp).sum(3, keepdims=True)
    ds, db = (gp * X).sum(3, keepdims=True), gp.sum(3, keepdims=True)
    err_ds, err_db = (Lc + 1) * U * A, Lc * U * B
    dgam = (ds - mean * db) * rstd
    canc = err_ds + np.abs(mean) * err_db + np.abs(db) * err_mean + 2 * U * (np.abs(mean * db) + np.abs(ds))     # of ds - mean db
    out['dgamma'] = (rstd * canc + (rel_rstd + 2 * U) * np.abs(dgam)).reshape(N, C)
    out['dbeta'] = np.maximum(err_db, 0).reshape(N, C)
    S1 = (gam4 * db).sum(2, keepdims=True)
    S2 = (gam4 * ds).sum(2, keepdims=True)
    aS1, aS2 = (np.abs(gam4 * db)).sum(2, keepdims=True), (np.abs(gam4 * ds)).sum(2, keepdims=True)
    err_S1 = (np.abs(gam4) * err_db).sum(2, keepdims=True) + (D + 1) * U * aS1
    err_S2 = (np.abs(gam4) * err_ds).sum(2, keepdims=True) + (D + 1) * U * aS2
    c2 = (S1 * mean - S2) * rstd ** 3 / n
    err_c2 = rstd ** 3 / n * (err_S1 * np.abs(mean) + err_S2 + np.abs(S1) * err_mean + 2 * U * (np.abs(S1 * mean) + np.abs(S2))) \
        + (3 * rel_rstd + 4 * U) * np.abs(c2)
    lead = np.abs(gp * gam4 * rstd)
    bgx = err_c2 * dev + 3 * U * np.abs(c2) * (np.abs(X) + np.abs(mean)) + np.abs(c2) * err_mean \
        + (err_S1 + (rel_rstd + 3 * U) * np.abs(S1)) * rstd / n + (rel_rstd + 4 * U) * lead + 2 * U * np.abs(ref['grad_x'].reshape(N, G, D, HW))
    out['grad_x'] = bgx.reshape(x.shape)
    return out


def _gn_case(N, C, G, HW, kind, relu, nulls, split=False, seed=0):
    lib, L = _L()
    rng = np.random.default_rng(seed)
    f = np.float32
    x = _gn_data(kind, N, C, G, HW, rng)
    gamma = None if 'gamma' in nulls else rng.normal(1.0, 0.5, C).astype(f)
    beta = None if 'beta' in nulls else rng.normal(0.0, 0.5, C).astype(f)
    D = C // G
    if kind == 'const' and beta is not None and relu:
        beta[C - D:] = 0                         # y == 0 there: the ReLU masks the whole group
    gy = rng.standard_normal((N, C, HW)).astype(f)
    want_gx = 'grad_x' not in nulls
    got = _gn_run(x, gamma, beta, G, relu, gy, want_gx, split)
    slices = L.kgdet_gn_act_slices(c_i64(N), c_i32(C), c_i32(G), c_i64(HW)) if split else 1
    mask = (got['y'] > 0) if relu else None
    ref = R.group_norm(x, gamma, beta, G, GN_EPS, relu_mask=mask, grad_y=gy)
    bounds = _gn_bounds(x, gamma, beta, G, gy, got, ref, relu, slices)
    if relu:     # the mask is the kernel's: where float64 is positive beyond the bound, fp32 must be too (and y >= 0 always)
        assert (got['y'] >= 0).all()
        pre = R.group_norm(x, gamma, beta, G, GN_EPS)['y']
        assert ((got['y'] > 0) | (pre <= bounds['y'])).all() and ((got['y'] == 0) | (pre >= -bounds['y'])).all()
    tag = 'N%d C%d G%d HW%d %s: ' % (N, C, G, HW, kind)
    worst = {}
    for name in ('y', 'mean', 'rstd', 'dgamma', 'dbeta') + (('grad_x',) if want_gx else ()):
        worst[name] = _ratio(got[name], ref[name], bounds[name], tag + name)
    assert max(worst.values()) <= 1.0, worst
    if kind == 'randn' and D * HW >= 64:      # the existing test's bar for this data, 2e-6 of the output's scale (a group of a
        # few values normalises to ~0: no scale to speak of)
        for name in ('y',) + (('grad_x',) if want_gx else ()):
            assert np.abs(got[name] - ref[name]).max() <= 2e-6 * np.abs(ref[name]).max(), name
    if kind == 'const':
        grp = (0, slice(C - D, C))
        b = np.zeros(C, f) if beta is None else beta
        assert (got['y'][grp] == b[C - D:, None]).all()                       # exactly beta
        assert _ulps(got['rstd'][G - 1], f(1.0 / math.sqrt(float(f(GN_EPS))))) <= 1
        assert got['mean'][G - 1] == 2.0
        for name in ('grad_x', 'dgamma', 'dbeta'):
            assert np.isfinite(got[name]).all()
        if relu and (b[C - D:] == 0).all():
            assert (got['dgamma'][grp] == 0).all() and (got['dbeta'][grp] == 0).all()
            if want_gx:
                assert (got['grad_x'][grp] == 0).all()
    return got, ref, bounds


GN_D = [1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 17, 24, 33, 64]
GN_HW = [1, 3, 63, 64, 65, 1050]
GN_NULLS = [(), ('gamma',), ('beta',), ('grad_x',), ('gamma', 'beta'), ('gamma', 'beta', 'grad_x'), ()]


def _gn_grid():
    cases = []
    for i, D in enumerate(GN_D):
        for j in range(3):      # three of the six map sizes per D, every size with every third D; data set, ReLU and NULLs cycle
            k = 3 * i + j
            cases.append((D, GN_HW[(i + 2 * j) % 6], ('randn', 'mean50', 'const')[(i + j) % 3], k % 2, GN_NULLS[k % 7]))
    return cases


@pytest.mark.parametrize('D,HW,kind,relu,nulls', _gn_grid())
def test_group_norm_channels_per_group(D, HW, kind, relu, nulls):
    """every wave schedule of the backward (wpc = 16 / D waves per channel, rounds of 16 channels beyond 16), 3 groups x 2 images"""
    _gn_case(2, 3 * D, 3, HW, kind, relu, nulls, seed=D * 7 + HW)


@pytest.mark.parametrize('kind', ['randn', 'mean50', 'const'])
def test_group_norm_single_workgroup(kind):
    _gn_case(1, 8, 1, 130, kind, 1, (), seed=3)                          # N * groups == 1


@pytest.mark.parametrize('HW', [8191, 8192, 8193, 16381])
def test_group_norm_at_the_slicing_threshold(HW):
    """D * HW = 65536 - D, 65536 (one workgroup), 65536 + D (5 slices) and a prime HW (8 ragged slices) through the _split
    entry points; the first two also through the plain ones, held to the same bar"""
    lib, L = _L()
    N, C, G = 1, 16, 2
    slices = L.kgdet_gn_act_slices(c_i64(N), c_i32(C), c_i32(G), c_i64(HW))
    assert (slices > 1) == (8 * HW > 65536) and (HW != 16381 or (slices == 8 and HW % 8))
    a, _, _ = _gn_case(N, C, G, HW, 'randn', 1, (), split=True, seed=HW)
    if slices == 1:
        b, _, _ = _gn_case(N, C, G, HW, 'randn', 1, (), split=False, seed=HW)
    _gn_case(N, C, G, HW, 'mean50', 0, ('grad_x',) if HW == 8193 else (), split=True, seed=HW + 1)


# ============================================================================================ GroupNorm, bf16
def _bf16_floor_ceil(v):
    """the bf16 values below and above each float64 (bf16 = the upper 16 bits of an fp32)"""
    lo32 = v.astype(np.float32)
    lo32 = np.where(lo32.astype(np.float64) > v, np.nextafter(lo32, np.float32(-np.inf)), lo32).astype(np.float32)     # fp32 floor
    bits = lo32.view(np.int32).astype(np.int64)
    trunc = (bits & ~0xffff)                                   # toward zero in bf16
    exact = ((bits & 0xffff) == 0) & (lo32.astype(np.float64) == v)
    away = np.where(exact, trunc, trunc + 0x10000)
    t = trunc.astype(np.int32).view(np.float32).astype(np.float64)
    a = away.astype(np.int32).view(np.float32).astype(np.float64)
    neg = lo32 < 0
    zero = lo32 == 0
    floor = np.where(neg, a, t)
    ceil = np.where(neg, t, a)
    tiny = float(np.array([0x10000], np.int32).view(np.float32)[0])
    ceil = np.where(zero & (v > 0), tiny, np.where(zero, 0.0, ceil))
    floor = np.where(zero, 0.0, floor)
    return floor, ceil


@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('C,G,HW,split', [(256, 32, 35, False), (256, 32, 40, False), (64, 4, 35, False), (64, 4, 40, False),
                                          (96, 32, 35, False), (96, 32, 40, False), (48, 1, 35, False), (48, 1, 40, False),
                                          (256, 32, 8401, True), (48, 1, 1399, True)])
def test_group_norm_bf16(C, G, HW, split, channels_last):
    """bf16 in and out, NCHW and channels-last: D == 8 (the 16-byte vector path), and D = 16, 3, 48 (the generic paths), HW odd
    and even, one sliced case each through _bf16_split.  Bar: the output is one of the two bf16 neighbours of the float64
    result computed from the bf16 input; a value within the fp32 error of the kernel's arithmetic (the y bound of the fp32
    kernels) of a bf16 value may fall on either side of it."""
    lib, L = _L()
    N = 2
    rng = np.random.default_rng(C + HW)
    xb = torch.from_numpy((3 * rng.standard_normal((N, C, HW)) + 1).astype(np.float32)).to(torch.bfloat16)
    gamma, beta = rng.normal(1.0, 0.5, C).astype(np.float32), rng.normal(0.0, 0.5, C).astype(np.float32)
    x64 = xb.double().numpy()
    slices = L.kgdet_gn_act_slices(c_i64(N), c_i32(C), c_i32(G), c_i64(HW))
    assert (slices > 1) == split
    for relu, use_gamma, use_beta in ((1, True, True), (0, True, False), (0, False, True)):
        g_, b_ = gamma if use_gamma else None, beta if use_beta else None
        ref = R.group_norm(x64, g_, b_, G, GN_EPS)
        bound = _gn_bounds(x64.astype(np.float32), g_, b_, G, None, None, ref, 0, slices)['y']
        xin = (xb.permute(0, 2, 1) if channels_last else xb).contiguous().cuda()
        n16 = xin.numel()
        out = torch.full((64 + n16 + 64,), 777.0, dtype=torch.bfloat16, device='cuda')
        dg = None if g_ is None else torch.from_numpy(g_).cuda()
        db = None if b_ is None else torch.from_numpy(b_).cuda()
        yp = ctypes.c_void_p(out.data_ptr() + 2 * 64)
        xp = ctypes.c_void_p(xin.data_ptr())
        if split:
            L.kgdet_gn_act_scratch_floats.restype = ctypes.c_size_t
            scratch = Guarded(L.kgdet_gn_act_scratch_floats(c_i64(N), c_i32(C), c_i32(G), c_i64(HW)))
            lib.check(L.kgdet_gn_act_forward_bf16_split(xp, c_i32(int(channels_last)), _ptr(dg), _ptr(db), c_i32(G), c_f(GN_EPS), c_i32(relu),
                                                        yp, scratch.ptr(), c_i64(N), c_i32(C), c_i64(HW), lib.current_stream()), 'gn_bf16_split')
            assert scratch.intact()
        else:
            lib.check(L.kgdet_gn_act_forward_bf16(xp, c_i32(int(channels_last)), _ptr(dg), _ptr(db), c_i32(G), c_f(GN_EPS), c_i32(relu), yp,
                                                  c_i64(N), c_i32(C), c_i64(HW), lib.current_stream()), 'gn_bf16')
        assert (out[:64] == 777.0).all() and (out[64 + n16:] == 777.0).all()
        y = out[64:64 + n16].double().cpu()
        y = (y.view(N, HW, C).permute(0, 2, 1) if channels_last else y.view(N, C, HW)).numpy()
        want = np.maximum(ref['y'], 0) if relu else ref['y']
        lo, _ = _bf16_floor_ceil(want - bound)
        _, hi = _bf16_floor_ceil(want + bound)
        bad = (y < lo) | (y > hi)
        # (how often the fp32 slack decided: most elements sit strictly between their two neighbours)
        print('relu %d gamma %d beta %d: %d of %d outside their two bf16 neighbours' % (relu, use_gamma, use_beta, bad.sum(), y.size))
        assert not bad.any()
