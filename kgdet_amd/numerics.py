"""The envelope of the fp16-part dense convolutions, checked: scan the operands, reroute one layer to bf16 parts, or raise.

The default forward arithmetic of the dense convolutions (kgdet_amd/conv1x1.py, csrc/dense_forward.hip) splits each operand into
two fp16 parts, the weights scaled by 2^8.  That is fp32-class only while

* a weight -- with a frozen BatchNorm folded in, w * s with s = gamma / sqrt(var + eps) -- stays within
  ``WEIGHT_LIMIT = 65504 / 2^8 = 255.875``, and
* an activation stays within ``ACT_LIMIT = 65504`` (up to ``ACT_CLAMP = 131008`` the two parts still hold 11 bits).

Outside it the kernels clamp and return finite numbers with status KGDET_OK: one running variance of 1e-12 in a checkpoint
makes a wrong channel, silently.  This module is the check:

``scan(tensors, scales, limits)``    one launch of csrc/range_scan.hip over any list of fp32 CUDA tensors, one read-back
``EnvelopeGuard(model)``             every weight the fp16-part route can serve, enumerated once; ``check()`` -> violations
``enforce(model)``                   the check + the policy ``KGDET_ENVELOPE`` = bf16 (default) | raise | warn | off; called by
                                     ``checkpoint.load_checkpoint`` and by ``runner.Runner`` at the end of every epoch
``audit(model, imgs)``               a diagnostic: one eval forward with the input activation of every dense convolution scanned

Policies: ``bf16`` routes each violating layer to bf16 parts (``conv1x1.set_bf16_parts``: no range limit, ~5e-6 of the output
scale) and warns once per layer; the route stays for the life of the weight.  ``raise`` raises ``EnvelopeError`` naming layers
and values, ``warn`` only warns, ``off`` does nothing at all -- the library is not even loaded.  A non-finite weight raises under
every policy but ``off``.

Not covered: activations in normal runs (nothing is added to the training step or the inference batch; use ``audit``), the
deformable convolutions' operands (dcn.py packs them on a path of its own) and gradients (bf16 parts already)."""
import collections
import os
import struct
import warnings
import weakref

import numpy as np
import torch

from . import _lib, conv1x1
from .conv1x1 import EnvelopeError    # noqa: F401  (public here)

WEIGHT_LIMIT = 65504.0 / 256.0     # |w s| 2^8 <= 65504: 255.875
WEIGHT_CLAMP = 131008.0 / 256.0    # beyond, the image holds a clamped weight
ACT_LIMIT = 65504.0
ACT_CLAMP = 131008.0
POLICIES = ('bf16', 'raise', 'warn', 'off')

# one row of the result: float32 max |v s| over the finite products, counts of non-finite products and of those beyond each limit
RECORD = np.dtype([('max', '<f4'), ('nonfinite', '<u4'), ('over1', '<u4'), ('over2', '<u4')])
_ROW_WORDS = 8

Scale = collections.namedtuple('Scale', 'gamma var eps inner')     # s[o] = gamma[o] / sqrt(var[o] + eps) (gamma None: 1 / sqrt)


def policy():
    p = os.environ.get('KGDET_ENVELOPE', 'bf16')
    if p not in POLICIES:
        raise ValueError('KGDET_ENVELOPE=%r: one of %s' % (p, ', '.join(POLICIES)))
    return p


def _bits(x):
    return struct.unpack('<I', struct.pack('<f', float(x)))[0]


def table_rows(tensors, scales, limits, blocks_of):
    """the host side of the device table of kgdet_range_scan_multi (include/kgdet_hip.h): int64 [n, 8] and the total block count"""
    n = len(tensors)
    scales = list(scales) if scales is not None else [None] * n
    if n and not isinstance(limits[0], (tuple, list)):
        limits = [tuple(limits)] * n
    if not (len(scales) == len(limits) == n):
        raise ValueError('one scale and one pair of limits per tensor')
    rows, first = np.zeros((n, _ROW_WORDS), dtype=np.int64), 0
    for i, (t, sc, (hi1, hi2)) in enumerate(zip(tensors, scales, limits)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError('scan takes contiguous fp32 CUDA tensors')
        count = t.numel()
        rows[i, 0], rows[i, 1] = t.data_ptr(), count
        if sc is not None:
            need = -(-count // int(sc.inner))
            for v in (sc.gamma, sc.var):
                if v is not None and not (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.numel() >= need):
                    raise ValueError('a row scale needs contiguous fp32 CUDA gamma / var of ceil(count / inner) elements')
            rows[i, 2] = int(sc.inner)
            rows[i, 3] = sc.gamma.data_ptr() if sc.gamma is not None else 0
            rows[i, 4] = sc.var.data_ptr()
            rows[i, 5] = _bits(sc.eps)
        rows[i, 6] = _bits(hi1) | (_bits(hi2) << 32)
        rows[i, 7] = first
        first += blocks_of(count)
    return rows, first


class _Table(object):
    """a device table + its record buffer; ``run()``: one launch, one read-back"""

    def __init__(self, tensors, scales, limits):
        L = conv1x1._library()
        rows, self.blocks = table_rows(tensors, scales, limits, L.kgdet_range_scan_blocks)
        self.n = len(tensors)
        dev = tensors[0].device
        self.table = torch.from_numpy(rows).to(dev)
        self.records = torch.empty((self.n, 4), dtype=torch.int32, device=dev)

    def launch(self):
        _lib.check(conv1x1._library().kgdet_range_scan_multi(self.table.data_ptr(), self.n, self.blocks, self.records.data_ptr(),
                                                             _lib.raw_stream(self.table.device.index)), 'range_scan_multi')
        return self.records

    def run(self):
        return self.launch().cpu().numpy().view(RECORD).reshape(self.n)


def scan(tensors, scales=None, limits=(WEIGHT_LIMIT, WEIGHT_CLAMP)):
    """``tensors``: contiguous fp32 CUDA tensors (any alignment of 4 bytes); ``scales``: None or, per tensor, None or a ``Scale``;
    ``limits``: one (hi1, hi2) pair for all or one per tensor.  -> numpy structured array (``RECORD``), one row per tensor."""
    tensors = list(tensors)
    if not tensors:
        return np.zeros(0, dtype=RECORD)
    with torch.cuda.device(tensors[0].device):
        return _Table(tensors, scales, limits).run()


# ---- the weights of a model that the fp16-part route can serve --------------------------------------------------------------
Layer = collections.namedtuple('Layer', 'name conv bn')      # bn: the frozen-statistics BatchNorm folded into conv, or None
Violation = collections.namedtuple('Violation', 'name weight max nonfinite over1 over2 limit')


def _servable(conv):
    """can `conv1x1.applicable` / `applicable_stride2` (or the subsampled stride-2 1x1 route of backbone._conv_bn) hold for some
    input of this plain convolution?  (the static half of those predicates)"""
    if not isinstance(conv, torch.nn.Conv2d) or conv.weight.dtype != torch.float32 or conv.groups != 1:
        return False
    O, C, kh, kw = conv.weight.shape
    if kh != kw or kh not in (1, 3) or tuple(conv.dilation) != (1, 1) or conv.padding_mode != 'zeros':
        return False
    stride, pad = tuple(conv.stride), tuple(conv.padding)
    if pad != (kh // 2, kh // 2):
        return False
    aligned = O % 16 == 0 and C % 16 == 0
    if stride == (1, 1):
        return aligned or (kh == 1 and (O * C) % 2 == 0)
    return stride == (2, 2) and ((kh == 3 and C % 16 == 0) or (kh == 1 and (aligned or (O * C) % 2 == 0)))


def enumerate_layers(model):
    """[Layer]: the backbone's conv + BatchNorm pairs (each once with its BatchNorm -- the folded images hold w s -- and once plain:
    a pair's first training step and a BatchNorm in training mode run unfolded), the plain convolutions `conv1x1.applicable` can
    hold for, and the stem"""
    from . import backbone
    BN = torch.nn.modules.batchnorm._BatchNorm
    layers, seen = [], set()

    def pair(name, conv, bn):
        if (id(conv) not in seen and type(conv) is torch.nn.Conv2d and conv.bias is None and _servable(conv)
                and isinstance(bn, BN) and bn.track_running_stats):
            layers.append(Layer(name + ' (folded)', conv, bn))

    for name, m in model.named_modules():
        prefix = name + '.' if name else ''
        if isinstance(m, backbone.BasicBlock):       # (its forward calls the modules themselves: MIOpen, no envelope)
            seen.update(id(c) for c in m.modules())
        elif isinstance(m, backbone.Bottleneck) and m.with_dcn:
            # conv1, conv3 and the downsample branch go through backbone.conv_bn as in the dense block; conv2 runs on the DCN
            # kernels and conv2_offset on torch's fp32 convolution: no envelope for those two
            pair(prefix + 'conv1', m.conv1, m.norm1)
            pair(prefix + 'conv3', m.conv3, m.norm3)
            seen.update(id(c) for c in (m.conv2, getattr(m, 'conv2_offset', None)) if c is not None)
        elif isinstance(m, torch.nn.Sequential):
            if len(m) == 2:                              # a downsample branch: Sequential(conv, BatchNorm)
                pair(prefix + '0', m[0], m[1])
        else:                                            # ResNet-style naming: conv<i> with bn<i> / norm<i> beside it
            for cname, conv in m.named_children():
                if cname.startswith('conv') and cname[4:].isdigit():
                    bn = getattr(m, 'bn' + cname[4:], None) or getattr(m, 'norm' + cname[4:], None)
                    pair(prefix + cname, conv, bn)
        if isinstance(m, backbone.ResNet):
            w = m.conv1.weight
            if tuple(w.shape) == (64, 3, 7, 7) and w.dtype == torch.float32:       # backbone._stem_conv: packed plain
                layers.append(Layer(prefix + 'conv1 (stem)', m.conv1, None))
                seen.add(id(m.conv1))
    for name, m in model.named_modules():
        if id(m) not in seen and _servable(m):
            seen.add(id(m))
            layers.append(Layer(name, m, None))
    return layers


class EnvelopeGuard(object):
    """``EnvelopeGuard(model).check()`` -> [Violation] of the model's current weights, from ONE scan launch and ONE read-back.  The
    layers are enumerated once; the device table holds the parameters' and buffers' addresses and is built again when one of
    them changes (``model.to(...)``, ``load_state_dict(assign=True)``)."""

    def __init__(self, model, scan_table=None):
        self.model = weakref.ref(model)
        self.layers = enumerate_layers(model)
        self._make_table = scan_table or _Table
        self._key = self._table = None
        self.launches = 0

    def _tensors(self):
        ts = []
        for l in self.layers:
            ts.append(l.conv.weight)
            if l.bn is not None:
                ts.extend([l.bn.weight, l.bn.running_var] if l.bn.affine else [l.bn.running_var])
        return ts

    def table(self):
        key = tuple((id(t), t.data_ptr()) for t in self._tensors())
        if self._table is None or key != self._key:
            tensors, scales = [], []
            for l in self.layers:
                w = l.conv.weight
                tensors.append(w.detach())
                scales.append(None if l.bn is None else Scale(
                    l.bn.weight.detach() if l.bn.affine else None, l.bn.running_var, float(l.bn.eps), w.numel() // w.shape[0]))
            self._table, self._key = self._make_table(tensors, scales, (WEIGHT_LIMIT, WEIGHT_CLAMP)), key
        return self._table

    def check(self):
        if not self.layers:
            return []
        rec = self.table().run()
        self.launches += 1
        out = []
        for l, r in zip(self.layers, rec):
            limit = 'nonfinite' if r['nonfinite'] else 'clamp' if r['over2'] else 'limit' if r['over1'] else None
            if limit is not None:
                out.append(Violation(l.name, l.conv.weight, float(r['max']), int(r['nonfinite']), int(r['over1']), int(r['over2']),
                                     limit))
        return out


def describe(v):
    if v.limit == 'nonfinite':
        return '%s: %d non-finite value(s)' % (v.name, v.nonfinite)
    return '%s: max |w s| = %.6g, %d value(s) beyond %.3f%s' % (
        v.name, v.max, v.over1, WEIGHT_LIMIT, ', %d beyond %.2f (clamped)' % (v.over2, WEIGHT_CLAMP) if v.over2 else '')


_guards = weakref.WeakKeyDictionary()     # model -> its guard
_warned = {}                              # id(weight) -> weakref: layers already warned about


def guard_for(model):
    g = _guards.get(model)
    if g is None:
        g = _guards[model] = EnvelopeGuard(model)
    return g


def _warn_once(v, text):
    key = id(v.weight)
    r = _warned.get(key)
    if r is None or r() is not v.weight:
        _warned[key] = weakref.ref(v.weight, lambda _r, key=key: _warned.pop(key, None))
        warnings.warn(text, RuntimeWarning, stacklevel=3)


def apply_policy(violations, mode=None, before_reroute=None):
    """act on ``violations`` (of ``EnvelopeGuard.check``) by the policy -> the violations whose layer was rerouted by THIS call.
    ``before_reroute()`` runs once before the first change of a route (the Runner retires its graphed step there)."""
    mode = mode or policy()
    if mode == 'off' or not violations:
        return []
    bad = [v for v in violations if v.limit == 'nonfinite']
    if bad:
        raise EnvelopeError('non-finite convolution weights: ' + '; '.join(describe(v) for v in bad))
    if mode == 'raise':
        raise EnvelopeError('convolution weights outside the envelope of the fp16-part kernels (|w s| <= %.3f): %s -- '
                            'KGDET_ENVELOPE=bf16 routes such layers to bf16 parts'
                            % (WEIGHT_LIMIT, '; '.join(describe(v) for v in violations)))
    if mode == 'warn':
        for v in violations:
            _warn_once(v, 'outside the envelope of the fp16-part convolutions, results of this layer are clamped: ' + describe(v))
        return []
    pending, done = [v for v in violations if not conv1x1.bf16_parts(v.weight)], set()
    if pending and before_reroute is not None:
        before_reroute()
    for v in pending:
        if id(v.weight) not in done:         # (a pair is listed folded and plain: one weight, one route)
            conv1x1.set_bf16_parts(v.weight, True)
            done.add(id(v.weight))
        _warn_once(v, 'outside the envelope of the fp16-part convolutions, this layer now runs on bf16 parts: ' + describe(v))
    return pending


def enforce(model, mode=None, before_reroute=None):
    """``guard.check()`` + the policy for ``model``; under ``off`` nothing is scanned (the library is not touched).
    -> (violations, rerouted)"""
    mode = mode or policy()
    if mode == 'off':
        return [], []
    violations = guard_for(model).check()
    return violations, apply_policy(violations, mode, before_reroute)


# ---- activations: a diagnostic pass ------------------------------------------------------------------------------------------
def audit(model, imgs, forward=None):
    """One eval forward of ``model`` (``forward(model, imgs)``, default ``model.extract_feat(imgs)`` or ``model(imgs)``) with the
    input activation of every dense convolution scanned against ACT_LIMIT / ACT_CLAMP -> [dict(name, shape, max, nonfinite,
    over_limit, over_clamp)] in call order.  ``name`` is the innermost running module and the call's ordinal inside it (the
    backbone's blocks call the kernels from their own forward).  Each call adds one scan launch; the records are read back
    once at the end.  The stem's 7x7 kernel reads the normalised image and is not among them."""
    names, stack, calls, keep = dict((m, n) for n, m in model.named_modules()), [], [], []
    hooks = []

    def enter(mod, _args):
        stack.append([names.get(mod, ''), 0])

    def leave(mod, _args, _out):
        if stack:
            stack.pop()

    for m in model.modules():
        hooks.append(m.register_forward_pre_hook(enter))
        hooks.append(m.register_forward_hook(leave))
    inner = conv1x1._apply

    def scanned(img, x, M, taps, *args, **kw):
        if x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel():
            t = _Table([x], None, (ACT_LIMIT, ACT_CLAMP))
            top = stack[-1] if stack else ['', 0]
            top[1] += 1
            calls.append(('%s#%d' % (top[0], top[1]), (tuple(x.shape), M, taps)))
            keep.append((t, t.launch()))
        return inner(img, x, M, taps, *args, **kw)

    was_training = model.training
    conv1x1._apply = scanned
    try:
        model.eval()
        with torch.no_grad():
            if forward is not None:
                forward(model, imgs)
            elif hasattr(model, 'extract_feat'):
                model.extract_feat(imgs)
            else:
                model(imgs)
    finally:
        conv1x1._apply = inner
        for h in hooks:
            h.remove()
        model.train(was_training)
    if not keep:
        return []
    rec = torch.cat([r for _, r in keep]).cpu().numpy().view(RECORD).reshape(len(keep))
    return [dict(name=n, shape=s, max=float(r['max']), nonfinite=int(r['nonfinite']), over_limit=int(r['over1']),
                 over_clamp=int(r['over2'])) for (n, s), r in zip(calls, rec)]
