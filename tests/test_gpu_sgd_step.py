"""csrc/optim.hip multi_clip_sgd (gradient clip + torch.optim.SGD as one pass) through the C ABI against the float64 reference
and the rounding bounds of tests/sgd_refs.py, then through DistOptimizerHook and runner.GraphedTrainStep on a toy model.

Outputs sit inside buffers of a canary value that must stay untouched, as in tests/test_gpu_step_kernels.py; the tables are
the ones tests/test_sgd_refs.py has already put the fp32 restatement of the kernel through.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import sgd_refs as S
from tests import step_refs as R
from tests.test_gpu_step_kernels import CANARY, Guarded, _L, _bit_equal, _ptr, _ratio, c_d, c_f, c_i32, c_i64

pytestmark = pytest.mark.gpu

U = R.U
f32 = np.float32


class Table(object):
    """a sgd_refs.HostTable on the device + the pointer table {param, grad, momentum buffer (0 with ``no_buf``), a canary
    buffer in the slot the kernel must ignore, numel, first block}"""

    def __init__(self, host, no_buf=False):
        lib, L = _L()
        self.h = host
        self.chunk = L.kgdet_optim_chunk()
        self.dev = {k: torch.from_numpy(host.host[k]).cuda() for k in 'pgb'}
        self.slot3 = torch.full((4096 + 128,), CANARY, dtype=torch.float32, device='cuda')
        first, rows = 0, []
        for i in host.rows:
            n = host.sizes[i]
            ptrs = [self.dev[k].data_ptr() + 4 * host.offs[k][i] for k in 'pgb']
            if no_buf:
                ptrs[2] = 0
            rows.append(ptrs + [self.slot3.data_ptr() + 4 * 64, n, first])
            first += (n + self.chunk - 1) // self.chunk
        self.blocks = first
        self.table = torch.tensor(rows, dtype=torch.int64).cuda()
        self.partial, self.norm = Guarded(first), Guarded(1)

    def upload(self, arrays=None):
        for k in 'pgb':
            self.dev[k].copy_(torch.from_numpy((arrays or self.h.host)[k]))

    def args(self):
        return ctypes.c_void_p(self.table.data_ptr()), c_i32(len(self.h.rows)), c_i64(self.blocks)

    def grad_norm(self):
        lib, L = _L()
        lib.check(L.kgdet_multi_grad_norm(*self.args(), self.partial.ptr(), self.norm.ptr(), lib.current_stream()), 'multi_grad_norm')
        return self.norm.view().clone()

    def clip_sgd(self, norm, max_norm, lr, momentum, dampening, wd, nesterov):
        lib, L = _L()
        lib.check(L.kgdet_multi_clip_sgd(*self.args(), _ptr(norm), c_f(max_norm), c_f(lr), c_d(momentum), c_d(dampening), c_f(wd),
                                         c_i32(int(nesterov)), lib.current_stream()), 'multi_clip_sgd')

    def clip_sgd_dev(self, norm, max_norm, sched, ring, nring, momentum, dampening, wd, nesterov):
        lib, L = _L()
        lib.check(L.kgdet_multi_clip_sgd_dev(*self.args(), _ptr(norm), c_f(max_norm), _ptr(sched),
                                             ctypes.c_void_p(ring.data_ptr()) if ring is not None else ctypes.c_void_p(0), c_i32(nring),
                                             c_d(momentum), c_d(dampening), c_f(wd), c_i32(int(nesterov)), lib.current_stream()),
                  'multi_clip_sgd_dev')

    def read(self):
        return {k: self.dev[k].cpu().numpy() for k in 'pgb'}


@functools.lru_cache(maxsize=None)
def _step_tables():
    host = S.step_table()
    return host, Table(host), Table(host, no_buf=True)


def _same_bits(a, b):
    return bool((a.view(np.int32) == b.view(np.int32)).all())


def _check_step(tb, before, after, norm, max_norm, lr, momentum, dampening, wd, nesterov, tag=''):
    h = tb.h
    for k in 'pgb':      # everything outside the table's tensors: canaries, and the tensor that has no row
        assert _same_bits(after[k][~h.inside[k]], before[k][~h.inside[k]]), k
    assert bool((tb.slot3 == CANARY).all())
    assert tb.partial.intact() and tb.norm.intact()
    p, g, b = h.gather(before)
    args = (norm, max_norm, lr, momentum, dampening, wd, nesterov)
    ref = S.clip_sgd_step(p, g, b, *args)
    bg, bb, bp = S.clip_sgd_bounds(p, g, b, *args)
    pa, ga, ba = h.gather(after)
    if R.clip_coef(norm, max_norm) >= 1.0:
        assert _same_bits(after['g'], before['g'])
    if momentum == 0:
        assert _same_bits(after['b'], before['b'])
    # k of each output (sgd_refs.clip_sgd_bounds): g 3 when scaled; buffer k_g + (2 with weight decay) + 4; the direction k_d,
    # k_b + 1 or, with Nesterov, k_d + k_b + 4; p one more for lr * direction -- (k + 1) U of the magnitudes entering the last
    # addition.  The float32 restatement of the expression measures 0.37 / 0.48 / 1.00 of these bounds (tests/test_sgd_refs.py).
    for name, got, want, bound in (('g', ga, ref[1], bg), ('buf', ba, ref[2], bb), ('p', pa, ref[0], bp)):
        assert _ratio(got, want, bound, tag + name) <= 1.0, name
    return ref


@pytest.mark.parametrize('max_norm', S.MAX_NORMS)              # inactive, active, no clipping and norm = NULL
@pytest.mark.parametrize('momentum,wd,dampening,nesterov', S.grid())
def test_clip_sgd_one_step(momentum, wd, dampening, nesterov, max_norm):
    host, with_buf, without = _step_tables()
    tb = without if momentum == 0 else with_buf                 # momentum 0: zero buffer pointers in the table
    tb.upload()
    norm_dev, norm = None, None
    if max_norm > 0:
        norm_dev = tb.grad_norm()
        norm = float(norm_dev)
        assert (R.clip_coef(norm, max_norm) < 1.0) == (max_norm < 1.0)
    before = tb.read()
    tb.clip_sgd(norm_dev, max_norm, S.LR, momentum, dampening, wd, nesterov)
    after = tb.read()
    _check_step(tb, before, after, norm, max_norm, S.LR, momentum, dampening, wd, nesterov)
    if wd == 0:      # g == buf == 0 and no weight decay: nothing to move, the parameter keeps its bits
        i, lo, hi = S.ZERO
        z = slice(host.offs['p'][i] + lo, host.offs['p'][i] + hi)
        assert _same_bits(after['p'][z], before['p'][z])
        zb = slice(host.offs['b'][i] + lo, host.offs['b'][i] + hi)
        assert (after['b'][zb] == 0).all()


def test_clip_sgd_rows_are_where_the_case_needs_them():
    """the table reaches what it is meant to reach: 304 rows, shifted rows 1, 2 and 3 floats past a 16-byte boundary in each
    buffer alone, more than one block per tensor, a tensor without a row"""
    host, tb, _ = _step_tables()
    assert len(host.rows) == 304 and len(host.sizes) == 305 and tb.blocks > len(host.rows)
    for k in 'pgb':
        for i, s in S.SHIFTS[k].items():
            assert (tb.dev[k].data_ptr() + 4 * host.offs[k][i]) % 16 == 4 * s
        others = [j for j in 'pgb' if j != k]
        alone = [s for i, s in S.SHIFTS[k].items() if all(i not in S.SHIFTS[j] for j in others)]
        assert sorted(alone) == [1, 2, 3], (k, alone)


def test_clip_sgd_steps_from_the_reference_state():
    """five consecutive steps, each from the float64 reference's state rounded to fp32, the clip alternating between inactive
    and active: the per-step bar stays the one-step bar"""
    host = S.step_table(seed=4)
    tb = Table(host)
    momentum, dampening, wd, nesterov = 0.9, 0.0, float(f32(1e-4)), False
    rng = np.random.default_rng(11)
    for t in range(1, 6):
        S.fresh_gradients(host, rng)
        tb.upload()
        norm_dev = tb.grad_norm()
        max_norm = 35.0 if t % 2 else 0.05
        assert (R.clip_coef(float(norm_dev), max_norm) < 1.0) == (max_norm < 1.0)
        before = tb.read()
        tb.clip_sgd(norm_dev, max_norm, S.LR, momentum, dampening, wd, nesterov)
        ref = _check_step(tb, before, tb.read(), float(norm_dev), max_norm, S.LR, momentum, dampening, wd, nesterov, 'step %d ' % t)
        host.scatter('p', ref[0].astype(f32))
        host.scatter('b', ref[2].astype(f32))


@pytest.mark.parametrize('t0', [0, 1000])
def test_device_schedule_over_two_wraps_of_the_ring(t0):
    """130 consecutive calls of kgdet_multi_clip_sgd_dev over a 64-slot page-locked ring with a different rate in every slot,
    from a fresh schedule and from a resumed one: bit-equal to kgdet_multi_clip_sgd on a copy with the same rates as arguments"""
    sizes = [1, 3, 255, 4097, 700, 64]
    shifts = dict(p={1: 1}, g={4: 3}, b={2: 2})
    A, B = (Table(S.HostTable(sizes, shifts, seed=5, lo=-3, hi=1)) for _ in range(2))
    momentum, dampening, wd, ring_n = 0.9, 0.0, float(f32(1e-4)), 64
    ring = torch.full((ring_n,), 7.0, dtype=torch.float32).pin_memory()
    sched = Guarded(4, fill=[0.5, -1.0, -2.0, float(t0)])
    norm = torch.tensor([30.0], dtype=torch.float32, device='cuda')
    inside = A.h.inside['g']
    pool = [torch.from_numpy(np.where(inside, np.random.default_rng(k).normal(size=inside.size) * 3, CANARY).astype(f32)).cuda()
            for k in range(4)]
    for k in range(1, 131):
        s = t0 + k
        lr = f32(5e-3 * (1 + s / 1000.0))
        ring[s % ring_n] = float(lr)
        for T in (A, B):
            T.dev['g'].copy_(pool[k % 4])
        A.clip_sgd_dev(norm, 0.5, sched.view(), ring, ring_n, momentum, dampening, wd, False)
        B.clip_sgd(norm, 0.5, float(lr), momentum, dampening, wd, False)
        torch.cuda.synchronize()          # (the ring slot is rewritten 64 steps on: the device has read it by then anyway)
    sc = sched.view().cpu().numpy()
    assert sc[3] == t0 + 130 and sc[0].view(np.int32) == lr.view(np.int32), sc
    assert sc[1] == -1.0 and sc[2] == -2.0          # (not SGD's slots)
    for key in 'pgb':
        assert _bit_equal(A.dev[key], B.dev[key]), key
    assert sched.intact() and bool((A.slot3 == CANARY).all())
    assert not _bit_equal(A.dev['g'], pool[130 % 4])           # (the clip was active)
    A.clip_sgd_dev(norm, 0.5, sched.view(), None, 0, momentum, dampening, wd, False)      # no ring: the learning rate stays
    B.clip_sgd(norm, 0.5, float(lr), momentum, dampening, wd, False)
    sc = sched.view().cpu().numpy()
    assert sc[3] == t0 + 131 and sc[0].view(np.int32) == lr.view(np.int32)
    for key in 'pgb':
        assert _bit_equal(A.dev[key], B.dev[key]), key


@pytest.mark.parametrize('route', ['args', 'dev'])
@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_non_finite_gradient_spreads_as_in_torch(bad, route):
    """one NaN / inf gradient element: which elements of p, grad and buffer end up NaN or infinite is what clip_grad_norm_ +
    torch.optim.SGD make of the same data on the CPU (arithmetic only: a NaN norm poisons everything, an infinite one zeroes
    the finite gradients)"""
    sizes = [5, 4097, 300]
    host = S.HostTable(sizes, dict(p={0: 1}), seed=9, lo=-3, hi=0)
    host.set_row('g', 1, 4000, 4001, bad)
    tb = Table(host)
    momentum, wd, max_norm = 0.9, float(f32(1e-4)), 1.0
    norm_dev = tb.grad_norm()
    if route == 'args':
        tb.clip_sgd(norm_dev, max_norm, S.LR, momentum, 0.0, wd, False)
    else:
        sched = torch.tensor([S.LR, 0, 0, 0], dtype=torch.float32, device='cuda')
        tb.clip_sgd_dev(norm_dev, max_norm, sched, None, 0, momentum, 0.0, wd, False)
    after = tb.read()
    params = []
    for i in host.rows:
        p = torch.nn.Parameter(torch.from_numpy(host.host['p'][host.offs['p'][i]:host.offs['p'][i] + sizes[i]].copy()))
        p.grad = torch.from_numpy(host.host['g'][host.offs['g'][i]:host.offs['g'][i] + sizes[i]].copy())
        params.append(p)
    opt = torch.optim.SGD(params, lr=S.LR, momentum=momentum, weight_decay=wd, foreach=False)
    for i, p in zip(host.rows, params):
        opt.state[p]['momentum_buffer'] = torch.from_numpy(host.host['b'][host.offs['b'][i]:host.offs['b'][i] + sizes[i]].copy())
    torch.nn.utils.clip_grad_norm_(params, max_norm=max_norm, norm_type=2, foreach=False)
    opt.step()
    want = dict(p=np.concatenate([p.detach().numpy() for p in params]), g=np.concatenate([p.grad.numpy() for p in params]),
                b=np.concatenate([opt.state[p]['momentum_buffer'].numpy() for p in params]))
    got = dict(zip('pgb', host.gather(after)))
    for k in 'pgb':
        assert (np.isnan(got[k]) == np.isnan(want[k])).all(), k
        assert (np.isinf(got[k]) == np.isinf(want[k])).all(), k
        assert _same_bits(after[k][~host.inside[k]], host.host[k][~host.inside[k]]), k
    assert np.isnan(got['p']).any()
    assert np.isnan(got['p']).all() == (bad != bad)


# ============================================================================================ hook and graphed step
def _toy(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.Tanh(), torch.nn.Linear(53, 11), torch.nn.Tanh(),
                               torch.nn.Linear(11, 7)).cuda().train()


def _toy_data(seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(29, 37, generator=g).cuda(), torch.randn(29, 7, generator=g).cuda()


def _toy_loss(model, x, y):
    return ((model(x) - y) ** 2).mean() * 8.0


def _torch_step(model, opt, loss, grad_clip):
    opt.zero_grad()
    loss.backward()
    raw = [p.grad.detach().clone() for p in model.parameters()]
    norm = torch.nn.utils.clip_grad_norm_(list(model.parameters()), **grad_clip)
    opt.step()
    return raw, float(norm)


@pytest.mark.parametrize('max_norm', [35.0, 0.5])               # inactive and active on the toy model's gradients
def test_hook_takes_the_fused_sgd_step(max_norm):
    """DistOptimizerHook with a plain torch.optim.SGD, as runner.build_optimizer makes it from the DeepFashion2 configs, against
    clip_grad_norm_ + torch on a replica that is given the same state before every step.  Each replica is within the one-step
    bounds of the float64 step evaluated with ITS gradients and norm (torch's norm kernel sums in another order than
    multi_sqnorm), so they agree within the sum of the two bounds + the float64 difference between the two norms' steps."""
    from kgdet_amd.dist import DistOptimizerHook
    clip = dict(max_norm=max_norm, norm_type=2)
    lr, momentum, wd = S.LR, 0.9, 1e-4
    A, B = _toy(), _toy()
    oa = torch.optim.SGD(A.parameters(), lr=lr, momentum=momentum, weight_decay=wd)
    ob = torch.optim.SGD(B.parameters(), lr=lr, momentum=momentum, weight_decay=wd)
    hook = DistOptimizerHook(grad_clip=clip)
    x, y = _toy_data()
    worst = dict(p=0.0, buf=0.0)
    raw_a = {}                                   # replica A's gradients as backward left them (the hook clips them in place)
    for p in A.parameters():
        p.register_post_accumulate_grad_hook(lambda q: raw_a.__setitem__(q, q.grad.detach().clone()))
    for step in range(5):
        with torch.no_grad():
            for pa, pb in zip(A.parameters(), B.parameters()):
                pb.copy_(pa)
                if step > 0:
                    ob.state[pb]['momentum_buffer'].copy_(oa.state[pa]['momentum_buffer'])
        before = [(p.detach().cpu().numpy(), None if step == 0 else oa.state[p]['momentum_buffer'].cpu().numpy())
                  for p in A.parameters()]
        hook.step(A, oa, _toy_loss(A, x, y))
        raw, norm_b = _torch_step(B, ob, _toy_loss(B, x, y), clip)
        if step == 0:
            assert hook._fused_sgd.fused_steps == 0 and hook._fused_sgd.last_norm is None      # (buffers are torch's to create)
            continue
        norm_a = float(hook._fused_sgd.last_norm)
        assert (R.clip_coef(norm_a, max_norm) < 1.0) == (max_norm < 1.0), norm_a
        for (p0, b0), g, pa, pb in zip(before, raw, A.parameters(), B.parameters()):
            ga, gb = raw_a[pa].cpu().numpy(), g.cpu().numpy()
            wdf = float(f32(wd))
            ra = S.clip_sgd_step(p0, ga, b0, norm_a, max_norm, lr, momentum, 0.0, wdf, False)
            rb = S.clip_sgd_step(p0, gb, b0, norm_b, max_norm, lr, momentum, 0.0, wdf, False)
            _, bba, bpa = S.clip_sgd_bounds(p0, ga, b0, norm_a, max_norm, lr, momentum, 0.0, wdf, False)
            _, bbb, bpb = S.clip_sgd_bounds(p0, gb, b0, norm_b, max_norm, lr, momentum, 0.0, wdf, False)
            bufa, bufb = oa.state[pa]['momentum_buffer'], ob.state[pb]['momentum_buffer']
            worst['p'] = max(worst['p'], _ratio(pa.detach().cpu().numpy(), ra[0], bpa, 'step %d p' % step))
            worst['buf'] = max(worst['buf'], _ratio(bufa.cpu().numpy(), ra[2], bba, 'step %d buf' % step))
            assert (np.abs(pa.detach().cpu().numpy().astype(np.float64) - pb.detach().cpu().numpy())
                    <= bpa + bpb + np.abs(ra[0] - rb[0])).all()
            assert (np.abs(bufa.cpu().numpy().astype(np.float64) - bufb.cpu().numpy()) <= bba + bbb + np.abs(ra[2] - rb[2])).all()
    assert worst['p'] <= 1.0 and worst['buf'] <= 1.0, worst
    assert hook._fused_sgd.fused_steps == 4            # the first went through torch
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa['param_groups'] == sb['param_groups'] and sa['state'].keys() == sb['state'].keys()
    for k in sa['state']:
        assert sa['state'][k].keys() == sb['state'][k].keys()
        assert sa['state'][k]['momentum_buffer'].shape == sb['state'][k]['momentum_buffer'].shape


def _toy_batch_processor(model, data, train_mode=True):
    loss = _toy_loss(model, data['img'], data['target'])
    return dict(loss=loss, log_vars={}, num_samples=data['img'].shape[0])


def test_graphed_train_step_takes_a_plain_sgd():
    """runner.GraphedTrainStep with a plain torch.optim.SGD: warm-up 2 + the step in its captured form + four replays, the rate
    halved before the third replay, against an eager loop of clip_grad_norm_ + torch's SGD over the same seven steps.
    Tolerance per tensor: 7 x the largest one-step bound of that tensor at the last step -- the one-step bound is per element,
    but from the second step on an element's gradient carries the rounding of every other element through the forward pass, so
    the per-step error of a tensor is taken at its largest element's.  An eager loop that misses the rate change must differ
    by more than 10 x as much."""
    from kgdet_amd import runner as rn
    from kgdet_amd.dist import DistOptimizerHook
    clip = dict(max_norm=35, norm_type=2)
    lr, momentum, wd = S.LR, 0.9, 1e-4
    x, y = _toy_data()
    A = _toy()
    oa = torch.optim.SGD(A.parameters(), lr=lr, momentum=momentum, weight_decay=wd)
    hook = DistOptimizerHook(grad_clip=clip)
    g = rn.GraphedTrainStep(A, oa, hook, dict(img=x, target=y), warmup=2, batch_processor=_toy_batch_processor)
    assert g.fused is hook._fused_sgd and g.lr_t is None
    for k in range(4):
        if k == 2:
            oa.param_groups[0]['lr'] *= 0.5
        out = g.step()
    torch.cuda.synchronize()
    assert torch.isfinite(out['loss']).item()
    assert float(hook._fused_sgd._sched[3]) == 5.0          # the captured-form step + four replays

    def eager(halve):
        M = _toy()
        opt = torch.optim.SGD(M.parameters(), lr=lr, momentum=momentum, weight_decay=wd)
        for k in range(7):
            if halve and k == 5:
                opt.param_groups[0]['lr'] *= 0.5
            before = [(p.detach().cpu().numpy(), None if k == 0 else opt.state[p]['momentum_buffer'].cpu().numpy())
                      for p in M.parameters()]
            raw, norm = _torch_step(M, opt, _toy_loss(M, x, y), clip)
        bounds = [S.clip_sgd_bounds(p0, gr.cpu().numpy(), b0, norm, 35.0, opt.param_groups[0]['lr'], momentum, 0.0,
                                    float(f32(wd)), False)[2] for (p0, b0), gr in zip(before, raw)]
        return M, bounds

    M, bounds = eager(True)
    W, _ = eager(False)
    for pa, pm, pw, bound in zip(A.parameters(), M.parameters(), W.parameters(), bounds):
        tol = 7 * float(bound.max())
        diff = float((pa.detach() - pm.detach()).abs().max())
        missed = float((pa.detach() - pw.detach()).abs().max())
        print('graphed against eager: %.3e (tolerance %.3e); against an eager loop without the rate change: %.3e' % (diff, tol, missed))
        assert diff <= tol
        assert missed > 10 * tol
