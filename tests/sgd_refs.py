"""float64 reference, fp32 restatement, rounding bounds and test tables of csrc/optim.hip multi_clip_sgd (gradient clip +
torch.optim.SGD as one pass).  Plain numpy, no GPU: tests/test_sgd_refs.py pins the reference to torch's own CPU operators and
shows that the fp32 restatement stays inside the bounds on the very tables tests/test_gpu_sgd_step.py uploads.
"""
import itertools

import numpy as np

from tests.step_refs import U, clip_coef, f64

CANARY = 12345.678


# ---------------------------------------------------------------------------------------------- the step
def clip_sgd_step(p, g, buf, norm, max_norm, lr, momentum, dampening, wd, nesterov):
    """clip_grad_norm_ (coefficient from the given total ``norm``) + one torch.optim.SGD step (torch/optim/sgd.py
    _single_tensor_sgd; no maximize) in float64.  Returns the new (p, g, buf); g is the clipped gradient the parameter's .grad
    holds afterwards (scaled only when the coefficient is not 1).  ``buf`` None with momentum != 0 is torch's FIRST step: the
    buffer is created as a copy of the gradient (no dampening); with momentum == 0 the buffer comes back as it went in."""
    p, g = f64(p), f64(g)
    coef = clip_coef(norm, max_norm)
    with np.errstate(all='ignore'):
        if not coef >= 1.0:
            g = g * coef
        d = g + p * wd if wd != 0 else g
        if momentum != 0:
            buf = d.copy() if buf is None else momentum * f64(buf) + (1.0 - dampening) * d
            d = d + momentum * buf if nesterov else buf
        elif buf is not None:
            buf = f64(buf)
        p = p - lr * d
    return p, g, buf


def clip_sgd_step_f32(p, g, buf, norm, max_norm, lr, momentum, dampening, wd, nesterov):
    """csrc/optim.hip multi_clip_sgd, expression by expression in numpy float32 (one rounding per operation, no fused
    multiply-add); momentum and 1 - dampening rounded from double once, as kgdet_multi_clip_sgd does"""
    f = np.float32
    p, g, buf = (np.asarray(a, f).copy() for a in (p, g, buf))
    coef = f(1.0)
    mu, w = f(momentum), f(1.0 - dampening)
    with np.errstate(all='ignore'):
        if max_norm > 0:
            coef = f(max_norm) / (f(norm) + f(1e-6))
            coef = f(1.0) if coef >= f(1.0) else coef
        if not coef >= f(1.0):
            g = g * coef
        d = g + p * f(wd) if f(wd) != 0 else g
        if mu != 0:
            buf = mu * buf + w * d
            d = d + mu * buf if nesterov else buf
        p = p - f(lr) * d
    return p, g, buf


def clip_sgd_bounds(p, g, buf, norm, max_norm, lr, momentum, dampening, wd, nesterov):
    """Absolute fp32 rounding bounds (bound_g, bound_buf, bound_p) of multi_clip_sgd around clip_sgd_step, counted as
    step_refs.clip_adam_bounds counts: (k + 1) * 2^-24 times the magnitude of the terms entering the output's last addition, k =
    the fp32 roundings of the kernel's expression in front of it (each has a relative error of at most 2^-24 of its own result,
    and every intermediate is at most the magnitude named).  lr and wd reach the kernel as floats: the caller passes values that
    are floats already, so they round nothing.
      g' = g coef              k_g = 3 when scaled (norm + 1e-6, the division, the product: clip_adam_bounds), else no
                               rounding: bit-equal
      d = g' + p wd            k_d = k_g + 2 (product, sum) with weight decay; magnitude D = |g'| + |p wd| (the sum may cancel)
      buf' = mu buf + w d      k_b = k_d + 4 (momentum to float, mu buf, 1 - dampening to float, w d; the sum is the + 1);
                               magnitude B = |mu buf| + w D
      dir                      momentum == 0: d itself, k = k_d, magnitude D
                               plain: buf', k = k_b + 1 (its sum), magnitude B
                               Nesterov: d + mu buf', k = k_d + (k_b + 1) + 3 (momentum to float again, the product, the
                               sum), magnitude D + |mu| B
      p' = p - lr dir          the error of dir enters as lr (k_dir + 1) 2^-24 |dir|_mag (+ 1: the product lr dir); the difference
                               rounds once, relative to |p'| <= |p| + S, S = lr |dir|_mag:
                               bound_p = 2^-24 (|p| + S) + (k_dir + 1) 2^-24 S  (<= (k_p + 1) 2^-24 (|p| + S), k_p = k_dir + 1)
    A fused multiply-add merges a product's rounding into the sum's: it only removes roundings, so the bounds hold either way.
    """
    p, g, buf = f64(p), f64(g), f64(buf)
    coef = clip_coef(norm, max_norm)
    scaled = not coef >= 1.0
    k_g = 3 if scaled else 0
    gs = g * coef if scaled else g
    D = np.abs(gs) + np.abs(wd * p)
    k_d = k_g + (2 if wd != 0 else 0)
    k_b = k_d + 4
    B = np.abs(momentum * buf) + abs(1.0 - dampening) * D
    if momentum == 0:
        k_dir, mag = k_d, D
    elif nesterov:
        k_dir, mag = k_d + (k_b + 1) + 3, D + abs(momentum) * B
    else:
        k_dir, mag = k_b + 1, B
    S = abs(lr) * mag
    bound_p = U * (np.abs(p) + S) + (k_dir + 1) * U * S
    bound_buf = (k_b + 1) * U * B if momentum != 0 else np.zeros_like(B)
    return (k_g + 1) * U * np.abs(gs), bound_buf, bound_p


# ---------------------------------------------------------------------------------------------- cases
MOMENTA, DECAYS, DAMPENINGS, NESTEROVS = (0.0, 0.9), (0.0, 1e-4), (0.0, 0.1), (False, True)
MAX_NORMS = (35.0, 0.05, 0.0)          # on the tables below: inactive, active, no clipping (norm = NULL)
LR = float(np.float32(5e-3))


def grid():
    """(momentum, wd, dampening, nesterov) -- wd as the float the kernel receives"""
    return [(mu, float(np.float32(wd)), damp, nes)
            for mu, wd, damp, nes in itertools.product(MOMENTA, DECAYS, DAMPENINGS, NESTEROVS)]


def torch_accepts(momentum, dampening, nesterov):
    """torch.optim.SGD: 'Nesterov momentum requires a momentum and zero dampening' (the kernel evaluates every combination)"""
    return not nesterov or (momentum > 0 and dampening == 0)


# ---------------------------------------------------------------------------------------------- tables
SPECIAL_SIZES = [1, 3, 255, 4095, 4096, 4097, 3 * 4096 + 5]


def table_sizes(big=20000 + 3, n_rows=304, seed=1):
    """the sizes of tests/test_gpu_step_kernels.py's Adam table: every tail length around a block of 4096, 304 rows (the binary
    search at its real depth), + one tensor that gets slices but no row"""
    rng = np.random.default_rng(seed)
    sizes = list(SPECIAL_SIZES) + [big] + [1, 2, 3, 5, 4096, 4097]
    sizes += [int(s) for s in rng.integers(1, 3000, n_rows - len(sizes))]
    return sizes + [777]


# floats past a 16-byte boundary, per buffer and row: rows 8..10 all three together, then each buffer alone with 1, 2 and 3
# (rows 12 / 13 are a whole block and a block + 1: the scalar path over a full block)
SHIFTS = dict(p={8: 1, 9: 2, 10: 3, 11: 1, 20: 2, 40: 3},
              g={8: 1, 9: 2, 10: 3, 12: 2, 21: 1, 41: 3},
              b={8: 1, 9: 2, 10: 3, 13: 3, 22: 1, 42: 2})


class HostTable(object):
    """Tensors of the given sizes as slices of three flat float32 buffers (param 'p', grad 'g', momentum buffer 'b') of CANARY,
    each buffer with its own offsets (``shifts[k][i]`` floats past a 16-byte boundary for row i of buffer k); rows in
    ``leave_out`` get slices but no table row.  ``host[k]``, ``offs[k]``, ``inside[k]`` (mask of the elements of rows)."""

    def __init__(self, sizes, shifts=None, leave_out=(), seed=0, lo=-6, hi=-1.5):
        shifts = shifts or {}
        self.sizes = list(sizes)
        self.rows = [i for i in range(len(sizes)) if i not in leave_out]
        self.offs, self.total = {}, {}
        for k in 'pgb':
            offs, at = [], 8
            for i, n in enumerate(sizes):
                at = (at + 3) // 4 * 4 + shifts.get(k, {}).get(i, 0)
                offs.append(at)
                at += n + 8
            self.offs[k], self.total[k] = offs, at + 8
        rng = np.random.default_rng(seed)
        self.host = {k: np.full(self.total[k], CANARY, np.float32) for k in 'pgb'}
        self.inside = {k: np.zeros(self.total[k], bool) for k in 'pgb'}
        for i, n in enumerate(sizes):
            vals = dict(g=rng.normal(size=n) * 10.0 ** rng.uniform(lo, hi, n),          # 1e-6 .. 10^hi within every tensor
                        p=rng.normal(size=n),
                        b=rng.normal(size=n) * 10.0 ** rng.uniform(lo, hi, n))
            for k in 'pgb':
                o = self.offs[k][i]
                self.host[k][o:o + n] = vals[k]
                if i in self.rows:
                    self.inside[k][o:o + n] = True

    def set_row(self, k, i, lo, hi, value):
        o = self.offs[k][i]
        self.host[k][o + lo:o + hi] = value

    def gather(self, arrays=None):
        """(p, g, b) of the table's rows, concatenated in row order"""
        arrays = arrays or self.host
        return tuple(np.concatenate([arrays[k][self.offs[k][i]:self.offs[k][i] + self.sizes[i]] for i in self.rows]) for k in 'pgb')

    def scatter(self, k, flat, arrays=None):
        arrays = arrays or self.host
        at = 0
        for i in self.rows:
            o, n = self.offs[k][i], self.sizes[i]
            arrays[k][o:o + n] = flat[at:at + n]
            at += n

    def grad_norm(self):
        return float(np.sqrt(np.sum(f64(self.gather()[1]) ** 2)))


ZERO = (7, 100, 400)          # row 7 (the 20003-element tensor), elements 100..399: g == buf == 0


def step_table(seed=3):
    """the table of the one-step and five-step cases: ||g|| ~ 4 (max_norm 35 leaves it, 0.05 clips)"""
    sizes = table_sizes()
    tb = HostTable(sizes, SHIFTS, leave_out=(len(sizes) - 1,), seed=seed)
    for k in 'gb':
        tb.set_row(k, *ZERO, 0)
    return tb


def fresh_gradients(tb, rng):
    """new gradients of the same kind into the rows of ``tb`` (the five-step case)"""
    n = int(tb.inside['g'].sum())
    tb.scatter('g', (rng.normal(size=n) * 10.0 ** rng.uniform(-6, -1.5, n)).astype(np.float32))
