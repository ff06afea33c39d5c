"""float64 references of the small kernels of the training step (csrc/optim.hip, smooth_l1.hip, focal.hip, group_norm.hip).

Plain numpy / CPU torch, no GPU: each function takes the kernel's fp32 inputs and evaluates the same operation in float64.
tests/test_step_refs.py pins them to torch's own CPU operators; tests/test_gpu_step_kernels.py holds the kernels to them.
The ``*_f32`` functions restate a kernel's expressions operation by operation in numpy float32: the bar where a formula
saturates in fp32 (focal loss outside |x| <= 80), and the CPU check that a derived rounding bound holds for a correct kernel.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of fp32: one correctly rounded operation has a relative error of at most U
FLT_MIN = np.float32(1.17549435e-38)


def f64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.float64)


# ---------------------------------------------------------------------------------------------- optimizer
def grad_norm(grads):
    """sqrt(sum g^2) over every tensor of ``grads``"""
    return math.sqrt(sum(float(np.sum(f64(g) ** 2)) for g in grads))


def clip_coef(norm, max_norm):
    """clip_grad_norm_'s coefficient max_norm / (norm + 1e-6) clamped to 1 (NaN stays NaN, as torch.clamp leaves it);
    1.0 when there is no clipping (no norm, or max_norm <= 0)"""
    if norm is None or not max_norm > 0:
        return 1.0
    with np.errstate(all='ignore'):
        c = np.float64(max_norm) / (np.float64(norm) + 1e-6)
    return float(c) if not c >= 1.0 else 1.0


def clip_adam_step(p, g, m, v, norm, max_norm, lr, beta1, beta2, eps, wd, t):
    """clip_grad_norm_ (coefficient from the given total ``norm``) + one torch.optim.Adam step (ORIGINAL mode: weight decay
    added to the gradient; no amsgrad / maximize) of step number ``t``.  Returns the new (p, g, m, v); g is the clipped
    gradient the parameter's .grad holds afterwards (scaled only when the coefficient is not 1)."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    coef = clip_coef(norm, max_norm)
    with np.errstate(all='ignore'):
        if not coef >= 1.0:
            g = g * coef
        gv = g + wd * p if wd != 0 else g
        m = m + (1.0 - beta1) * (gv - m)
        v = beta2 * v + (1.0 - beta2) * gv * gv
        bc1, bc2s = 1.0 - beta1 ** t, math.sqrt(1.0 - beta2 ** t)
        p = p - (lr / bc1) * m / (np.sqrt(v) / bc2s + eps)
    return p, g, m, v


def clip_adam_step_f32(p, g, m, v, norm, max_norm, lr, beta1, beta2, eps, wd, bc1, bc2s):
    """csrc/optim.hip multi_clip_adam, expression by expression in numpy float32 (no fused multiply-add)"""
    f = np.float32
    p, g, m, v = (np.asarray(a, f).copy() for a in (p, g, m, v))
    coef = f(1.0)
    with np.errstate(all='ignore'):
        if max_norm > 0:
            coef = f(max_norm) / (f(norm) + f(1e-6))
            coef = f(1.0) if coef >= f(1.0) else coef
        if not coef >= f(1.0):
            g = g * coef
        gv = g + p * f(wd) if f(wd) != 0 else g
        w1, w2, b2 = f(1.0 - beta1), f(1.0 - beta2), f(beta2)
        m = m + w1 * (gv - m) if w1 < f(0.5) else gv - (gv - m) * (f(1.0) - w1)
        v = b2 * v + w2 * gv * gv
        denom = np.sqrt(v) / f(bc2s) + f(eps)
        p = p - (f(lr) / f(bc1)) * m / denom
    return p, g, m, v


# ---------------------------------------------------------------------------------------------- smooth L1
def smooth_l1_terms(pred, target, beta, divisor):
    """x = p / d - t / d and l(|x|) = |x| < beta ? 0.5 x^2 / beta : |x| - 0.5 beta, element-wise in float64"""
    with np.errstate(all='ignore'):
        x = f64(pred) / divisor - f64(target) / divisor
        a = np.abs(x)
        return x, np.where(a < beta, 0.5 * a * a / beta, a - 0.5 * beta)


def _weighted(weight, val):
    """weight * val, a zero weight giving exactly zero whatever val is (the kernel does not read where a wave weighs zero)"""
    if weight is None:
        return val
    w = f64(weight)
    with np.errstate(all='ignore'):
        return np.where(w != 0, w * val, 0.0)


def smooth_l1_sum(pred, target, weight, beta, divisor):
    _, l = smooth_l1_terms(pred, target, beta, divisor)
    return float(np.sum(_weighted(weight, l)))


def smooth_l1_grad(pred, target, weight, grad_sum, beta, divisor):
    """d sum / d pred * grad_sum: the quadratic branch gives x / beta, the linear one sign(x) (0 at 0)"""
    x, _ = smooth_l1_terms(pred, target, beta, divisor)
    with np.errstate(all='ignore'):
        dl = np.where(np.abs(x) < beta, x / beta, np.sign(x))
        return _weighted(weight, dl) * (float(grad_sum) / divisor)


def smooth_l1_branch_window(pred, target, beta, divisor):
    """elements so close to |x| == beta that fp32 may put them on either branch: ||x| - beta| < 2^-20 (|p| + |t|) / |d|"""
    x, _ = smooth_l1_terms(pred, target, beta, divisor)
    with np.errstate(all='ignore'):
        return np.abs(np.abs(x) - beta) < 2.0 ** -20 * (np.abs(f64(pred)) + np.abs(f64(target))) / abs(divisor)


def smooth_l1_f32(pred, target, weight, grad_sum, beta, divisor):
    """csrc/smooth_l1.hip element by element in numpy float32: (weighted loss terms, grad_pred); no wave skip"""
    f = np.float32
    p, t = np.asarray(pred, f), np.asarray(target, f)
    w = f(1.0) if weight is None else np.asarray(weight, f)
    beta, d, g = f(beta), f(divisor), f(grad_sum)
    x = p / d - t / d
    a = np.abs(x)
    l = np.where(a < beta, f(0.5) * a * a / beta, a - f(0.5) * beta)
    dl = np.where(a < beta, x / beta, np.sign(x)).astype(f)
    return (l * w).astype(f), (g * w * dl / d).astype(f)


# ---------------------------------------------------------------------------------------------- sigmoid focal loss
def _focal_classes(target, num_classes):
    """c1 / c2 of the reference kernel: the positive class of a row (label t in 1..C -> class t - 1) and its negatives
    (every other class of a row with t >= 0; t < 0 ignores the row, t > C makes every class a negative)"""
    t = np.asarray(target, np.int64)[:, None]
    d = np.arange(num_classes, dtype=np.int64)[None, :]
    c1 = t == d + 1
    return c1, (t >= 0) & ~c1


def focal_forward(logits, target, gamma, alpha):
    """-alpha (1 - p)^gamma log p for the positive class, -(1 - alpha) p^gamma log(1 - p) for the negatives, float64
    (the formula of the reference's CUDA kernel and of py_sigmoid_focal_loss)"""
    x = f64(logits)
    c1, c2 = _focal_classes(target, x.shape[1])
    logp, log1mp = -np.logaddexp(0.0, -x), -np.logaddexp(0.0, x)
    p, q = np.exp(logp), np.exp(log1mp)
    return np.where(c1, -alpha * q ** gamma * logp, 0.0) + np.where(c2, -(1.0 - alpha) * p ** gamma * log1mp, 0.0)


def focal_backward(logits, target, d_losses, gamma, alpha):
    x = f64(logits)
    c1, c2 = _focal_classes(target, x.shape[1])
    logp, log1mp = -np.logaddexp(0.0, -x), -np.logaddexp(0.0, x)
    p, q = np.exp(logp), np.exp(log1mp)
    g1 = -alpha * q ** gamma * (q - gamma * p * logp)
    g2 = -(1.0 - alpha) * p ** gamma * (gamma * q * log1mp - p)
    return (np.where(c1, g1, 0.0) + np.where(c2, g2, 0.0)) * f64(d_losses)


def _focal_f32_parts(logits, gamma):
    f, d = np.float32, np.float64
    x = np.asarray(logits, f)
    with np.errstate(all='ignore'):
        p = (1.0 / (1.0 + np.exp(-x).astype(d))).astype(f)
        one_m_p = (1.0 - p.astype(d)).astype(f)
        logp = np.log(np.maximum(p, FLT_MIN))
        ge = (x >= 0).astype(d)
        inner = (x.astype(d) - 2.0 * x.astype(d) * ge).astype(f)
        nsp = -1.0 * x.astype(d) * ge - np.log((1.0 + np.exp(inner).astype(d)).astype(f)).astype(d)     # double
        pow_q, pow_p = np.power(one_m_p, f(gamma)), np.power(p, f(gamma))
    return x, p, logp, nsp, pow_q, pow_p


def focal_forward_f32(logits, target, gamma, alpha):
    """csrc/focal.hip focal_forward with its float / double promotions, in numpy (float libm calls on float32 arrays)"""
    f, d = np.float32, np.float64
    x, p, logp, nsp, pow_q, pow_p = _focal_f32_parts(logits, gamma)
    c1, c2 = (c.astype(f) for c in _focal_classes(target, x.shape[1]))
    zn, zp = f(1.0 - d(f(alpha))), f(alpha)
    with np.errstate(all='ignore'):
        term1 = pow_q * logp
        term2 = (pow_p.astype(d) * nsp).astype(f)
        return (-c1 * term1 * zp) + (-c2 * term2 * zn)


def focal_backward_f32(logits, target, d_losses, gamma, alpha):
    f, d = np.float32, np.float64
    x, p, logp, nsp, pow_q, pow_p = _focal_f32_parts(logits, gamma)
    c1, c2 = (c.astype(f) for c in _focal_classes(target, x.shape[1]))
    zn, zp = f(1.0 - d(f(alpha))), f(alpha)
    with np.errstate(all='ignore'):
        term1 = (pow_q.astype(d) * (1.0 - p.astype(d) - (p * f(gamma) * logp).astype(d))).astype(f)
        term2 = (pow_p.astype(d) * (nsp * (1.0 - p.astype(d)) * d(f(gamma)) - p.astype(d))).astype(f)
        return ((-c1 * term1 * zp) + (-c2 * term2 * zn)) * np.asarray(d_losses, f)


# ---------------------------------------------------------------------------------------------- GroupNorm (+ ReLU)
def group_norm(x, gamma, beta, groups, eps, relu_mask=None, grad_y=None, want_grad_x=True):
    """torch.nn.functional.group_norm on float64 CPU tensors (+ ReLU as the given mask of the kernel's own fp32 output: an
    element within rounding of zero may flip in float64).  x [N, C, HW].  Returns a dict of float64 numpy arrays: y, mean, rstd
    [N * groups], and with ``grad_y``: grad_x, dgamma [N, C], dbeta [N, C] (per-image rows, as the kernel leaves them)."""
    import torch.nn.functional as F
    xd = torch.as_tensor(f64(x)).clone().requires_grad_(grad_y is not None)
    N, C, HW = xd.shape
    gd = torch.ones(C, dtype=torch.float64) if gamma is None else torch.as_tensor(f64(gamma)).clone()
    bd = torch.zeros(C, dtype=torch.float64) if beta is None else torch.as_tensor(f64(beta)).clone()
    # per-image rows of dgamma / dbeta: one copy of the affine parameters per image
    gN = gd[None].repeat(N, 1).requires_grad_(grad_y is not None)
    bN = bd[None].repeat(N, 1).requires_grad_(grad_y is not None)
    y = F.group_norm(xd, groups, None, None, eps) * gN[:, :, None] + bN[:, :, None]
    if relu_mask is not None:
        y = y * torch.as_tensor(np.asarray(relu_mask, np.float64))
    xg = xd.detach().reshape(N * groups, -1)
    mean = xg.mean(1)
    out = dict(y=y.detach().numpy(), mean=mean.numpy(),
               rstd=(1.0 / torch.sqrt(((xg - mean[:, None]) ** 2).mean(1) + eps)).numpy())
    if grad_y is not None:
        y.backward(torch.as_tensor(f64(grad_y)))
        out.update(grad_x=xd.grad.numpy(), dgamma=gN.grad.numpy(), dbeta=bN.grad.numpy())
    return out


# ---------------------------------------------------------------------------------------------- bounds and shared inputs
def clip_adam_bounds(p, g, m, v, norm, max_norm, lr, beta1, beta2, eps, wd, t):
    """Absolute fp32 rounding bounds (bound_g, bound_m, bound_v, bound_p) of csrc/optim.hip:113-127 around clip_adam_step, each
    (k + 1) * 2^-24 times the magnitude of the terms entering the output's last addition, k = the number of fp32 roundings of
    the kernel's expression in front of it (every rounding has a relative error of at most 2^-24 of its own result, and every
    intermediate here is at most that magnitude, or twice it times a weight below one half):
      g' = g coef            k_g = 3 when scaled (norm + 1e-6, the division, the product), else no rounding: bit-equal
      gv = g' + p wd         k_gv = k_g + 2 (product, sum) with weight decay; magnitude G = |g'| + |p wd| (the sum may cancel)
      m' = lerp(m, gv, w1)   k_m = k_gv + 4 (1 - beta1 to float, gv - m, the product, the sum); the w1 >= 0.5 form has one more
                             (1.0f - w1); magnitude M = max(|m|, G)
      v' = b2 v + w2 gv gv   k_v = 2 k_gv + 6 (beta2 and 1 - beta2 to float, three products, the sum); all terms >= 0: magnitude
                             V = b2 v + w2 G^2 (= v' unless gv cancels)
      p' = p - s m' / den    the error of m' enters as s bound_m / den; den = sqrt(v') / c2 + eps carries bound_v / (2 sqrt(v') c2)
                             and 4 roundings (sqrt, sqrt(1 - beta2^t) to float, the division, + eps); s = lr / c1 has 2 (1 - beta1^t to
                             float, the division); product and quotient 2; the difference 1, relative to |p'| <= |p| + |step|.
                             With |step| taken at M -- S = s M / den, because the error of m' is relative to M, not to |m'| --
                             bound_p = 2^-24 (|p| + S) + s bound_m / den + S (err_den / den + 8 * 2^-24); without cancellation
                             in gv this is (k_p + 1) 2^-24 (|p| + S), k_p = (k_m + 1) + (k_v + 1) / 2 + 8.
    """
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    coef = clip_coef(norm, max_norm)
    scaled = not coef >= 1.0
    k_g = 3 if scaled else 0
    gs = g * coef if scaled else g
    G = np.abs(gs) + np.abs(wd * p)
    k_gv = k_g + (2 if wd != 0 else 0)
    M = np.maximum(np.abs(m), G)
    k_m = k_gv + (4 if np.float32(1.0 - beta1) < 0.5 else 5)
    k_v = 2 * k_gv + 6
    pn, gn, mn, vn = clip_adam_step(p, g, m, v, norm, max_norm, lr, beta1, beta2, eps, wd, t)
    bound_m = (k_m + 1) * U * M
    bound_v = (k_v + 1) * U * (beta2 * v + (1.0 - beta2) * G * G)
    c2, s = math.sqrt(1.0 - beta2 ** t), lr / (1.0 - beta1 ** t)
    den = np.sqrt(vn) / c2 + eps
    with np.errstate(all='ignore'):
        err_den = np.where(vn > 0, bound_v / (2.0 * np.sqrt(vn) * c2), np.sqrt(bound_v) / c2) + 4 * U * den
    S = s * M / den
    bound_p = U * (np.abs(p) + S) + s * bound_m / den + S * (err_den / den + 8 * U)
    return (k_g + 1) * U * np.abs(gn), bound_m, bound_v, bound_p


def dense_smooth_l1_inputs(seed=0, rows=33600, cols=588):
    """The dense keypoint targets of a five-level head: pred = 300 + 40 randn, target = pred + 20 randn (every third row equal to
    the prediction: exact zeros of the difference), a weight that is zero except for 12 whole rows and a few single elements.
    float32 arrays [rows, cols]."""
    rng = np.random.default_rng(seed)
    pred = (300 + 40 * rng.standard_normal((rows, cols), dtype=np.float32)).astype(np.float32)
    target = (pred + 20 * rng.standard_normal((rows, cols), dtype=np.float32)).astype(np.float32)
    target[::3] = pred[::3]
    weight = np.zeros((rows, cols), np.float32)
    r = np.arange(rows)
    pos = np.concatenate([rng.choice(r[r % 3 == 0], 3, replace=False), rng.choice(r[r % 3 != 0], 9, replace=False)])
    weight[pos] = (0.05 + rng.random((12, cols))).astype(np.float32)
    for _ in range(7):
        weight[rng.integers(rows), rng.integers(cols)] = np.float32(0.5 + rng.random())
    return pred, target, weight


def zero_weight_waves(weight):
    """flat index mask of the elements whose aligned run of 64 (a wave of the kernel's grid-stride loop) weighs zero entirely"""
    w = np.asarray(weight).reshape(-1)
    n = w.size
    pad = np.concatenate([w, np.zeros((-n) % 64, w.dtype)])       # (a ragged last wave has fewer lanes: all of THEM must be zero)
    return np.repeat((pad.reshape(-1, 64) == 0).all(1), 64)[:n]
