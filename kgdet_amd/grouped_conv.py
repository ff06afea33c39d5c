"""Grouped 3x3 convolutions (padding 1, dilation 1, stride 1 or 2), fp32 NCHW, on the HIP kernels of csrc/grouped_conv.hip:
the ``conv2`` of a ResNeXt bottleneck (kgdet_amd/backbone.py), 4, 8, 16 or 32 channels per group.

``conv3x3(x, weight, stride)`` equals ``F.conv2d(x, weight, None, stride, 1, 1, groups)`` for a ``[C, cpg, 3, 3]`` weight with
``groups = C // cpg``, forward and both gradients, in exact fp32 arithmetic (one FMA chain per result, no atomics: equal bits
from call to call).  ``conv3x3_bias_act`` is the inference call with the folded-BatchNorm shift and the ReLU in the store.

``conv3x3_nhwc(x, weight, stride, bias, relu)`` is the bf16 autocast inference call on channels-last storage
(csrc/grouped_conv_nhwc.hip, MFMA with fp32 accumulation), opt-in: ``KGDET_GROUPED_CONV_BF16`` / ``BF16``."""
import ctypes
import os as _os

import torch

from . import _lib


# ---- switches (the other setting of each, and who uses it) ----------------------------------------------------------------
# KGDET_GROUPED_CONV=0 / ENABLED = False: every grouped convolution stays on torch (the tests and tools/time_grouped_conv.py
# compare the two routes)
ENABLED = _os.environ.get('KGDET_GROUPED_CONV', '1') != '0'
# (channels per group, stride) classes that stay on torch by default: forward + grad_input + grad_weight of the route measured
# slower than torch's there at batch 2, 800 x 1344 (tools/time_grouped_conv.py, the table in the README): 16 and 32 channels per
# group.  KGDET_GROUPED_CONV=force / FORCE = True routes them too (the correctness tests, the timing tool)
TORCH_CLASSES = frozenset([(16, 1), (16, 2), (32, 1), (32, 2)])
FORCE = _os.environ.get('KGDET_GROUPED_CONV') == 'force'

# KGDET_GROUPED_CONV_BF16 / BF16: the bf16 channels-last inference route (csrc/grouped_conv_nhwc.hip) -- unset or 0: off, the
# default (bf16 autocast inference keeps every grouped convolution on torch); 1: every (channels per group, stride) class
# except TORCH_CLASSES_BF16; force: every class.  KGDET_GROUPED_CONV=0 turns this route off as well.  tools/test.py
# --grouped-bf16 sets the attribute.
def parse_bf16(value):
    """the setting of KGDET_GROUPED_CONV_BF16 / --grouped-bf16: '0' (also None or ''), '1' or 'force'"""
    value = '0' if value in (None, '') else str(value)
    if value not in ('0', '1', 'force'):
        raise ValueError("KGDET_GROUPED_CONV_BF16 is 0, 1 or force, not %r" % (value,))
    return value


BF16 = parse_bf16(_os.environ.get('KGDET_GROUPED_CONV_BF16'))
# classes where the route did not measure faster than F.conv2d (+ kgdet_bias_act) beyond the spread of the timing windows
# (tools/time_grouped_conv.py --bf16, the table in the README); empty while unmeasured
TORCH_CLASSES_BF16 = frozenset()

CPG = (4, 8, 16, 32)
calls = {'forward': 0, 'bias_act': 0, 'grad_input': 0, 'grad_weight': 0}     # launches per entry point (the tests read them)
calls_nhwc = {'raw': 0, 'bias_act': 0}                                        # launches of the bf16 channels-last entry point

_vp, _i32, _i64, _sz, _int = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_int
_PROTOTYPES = (
    ('kgdet_gconv3x3_forward', _int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    ('kgdet_gconv3x3_grad_input', _int, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp]),
    ('kgdet_gconv3x3_workspace_bytes', _sz, [_i64, _i32, _i32, _i32, _i32, _i32]),
    ('kgdet_gconv3x3_grad_weight', _int, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    ('kgdet_gconv3x3_nhwc_bf16', _int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp]))
_L = None
_sizes = {}


def library():
    """the loaded library with the prototypes of the grouped entry points declared"""
    global _L
    if _L is None:
        L = _lib.lib()
        for name, res, args in _PROTOTYPES:
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _L = L
    return _L


def reset_calls():
    for k in calls:
        calls[k] = 0


def reset_calls_nhwc():
    for k in calls_nhwc:
        calls_nhwc[k] = 0


def applicable(x, weight, stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1):
    """the envelope of the kernels: a float32 contiguous NCHW tensor on the GPU, a float32 [C, cpg, 3, 3] weight with cpg in
    {4, 8, 16, 32} and C = groups * cpg, stride 1 or 2 (both directions alike), padding 1, dilation 1, no autocast.  One group
    is a dense convolution: it is taken when asked for, but backbone._conv_bn asks the dense routes first."""
    if not (ENABLED and torch.is_tensor(x) and torch.is_tensor(weight) and x.is_cuda and weight.is_cuda
            and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.is_contiguous()
            and shape_ok(x.shape, weight.shape, stride, padding, dilation, groups)):
        return False
    stride = stride if isinstance(stride, int) else stride[0]
    return (FORCE or (weight.shape[1], stride) not in TORCH_CLASSES) and not torch.is_autocast_enabled()


def shape_ok(x_shape, w_shape, stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1):
    """the shape part of `applicable` (device, dtype and layout aside)"""
    def pair(v):
        return (v, v) if isinstance(v, int) else tuple(v)
    if len(x_shape) != 4 or len(w_shape) != 4:
        return False
    C, cpg = w_shape[0], w_shape[1]
    return (tuple(w_shape[2:]) == (3, 3) and cpg in CPG and groups >= 1 and C == groups * cpg and x_shape[1] == C
            and pair(stride) in ((1, 1), (2, 2)) and pair(padding) == (1, 1) and pair(dilation) == (1, 1)
            and min(x_shape) >= 1 and x_shape[0] <= 65535 and C * (cpg // 4) <= 65535
            and x_shape[2] * x_shape[3] < 2 ** 31)


def applicable_bf16(x, weight, stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1):
    """the envelope of the bf16 inference kernel, and its switch: a bfloat16 tensor on the GPU contiguous in channels_last, a
    bfloat16 [C, cpg, 3, 3] weight contiguous in channels_last (its storage is the kernel's [C][3][3][cpg]), `shape_ok` and
    C % 8 == 0, autograd off"""
    if not (ENABLED and BF16 != '0' and torch.is_tensor(x) and torch.is_tensor(weight) and x.is_cuda and weight.is_cuda
            and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and not torch.is_grad_enabled()
            and shape_ok(x.shape, weight.shape, stride, padding, dilation, groups) and weight.shape[0] % 8 == 0
            and x.is_contiguous(memory_format=torch.channels_last)
            and weight.is_contiguous(memory_format=torch.channels_last)
            and x.data_ptr() % 16 == 0 and weight.data_ptr() % 16 == 0):
        return False
    stride = stride if isinstance(stride, int) else stride[0]
    return BF16 == 'force' or (weight.shape[1], stride) not in TORCH_CLASSES_BF16


def conv3x3_nhwc(x, weight, stride, bias=None, relu=False):
    """bf16 inference of an x that `applicable_bf16` accepted: the raw convolution (no bias, no ReLU: what the fused conv3
    kernel takes with in_bias), or ``[relu](conv + bias[c])`` with the fp32 bias in the store -- a channels-last bf16 tensor"""
    B, C, H, W = x.shape
    y = torch.empty(_out_shape(x, stride), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    _lib.check(library().kgdet_gconv3x3_nhwc_bf16(
        x.data_ptr(), weight.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(), B, C, weight.shape[1], H, W,
        int(stride), 1 if relu else 0, _lib.raw_stream(x.device.index)), 'gconv3x3_nhwc_bf16')
    calls_nhwc['raw' if bias is None and not relu else 'bias_act'] += 1
    return y


def _out_shape(x, stride):
    B, C, H, W = x.shape
    return B, C, (H - 1) // stride + 1, (W - 1) // stride + 1


def forward(x, weight, stride, bias=None, relu=False):
    y = torch.empty(_out_shape(x, stride), dtype=torch.float32, device=x.device)
    B, C, H, W = x.shape
    _lib.check(library().kgdet_gconv3x3_forward(
        x.data_ptr(), weight.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(), B, C, weight.shape[1], H, W,
        stride, 1 if relu else 0, _lib.raw_stream(x.device.index)), 'gconv3x3_forward')
    calls['forward' if bias is None and not relu else 'bias_act'] += 1
    return y


def grad_input(gy, weight, x_shape, stride):
    B, C, H, W = x_shape
    gx = torch.empty(x_shape, dtype=torch.float32, device=gy.device)
    _lib.check(library().kgdet_gconv3x3_grad_input(
        gy.data_ptr(), weight.data_ptr(), gx.data_ptr(), B, C, weight.shape[1], H, W, stride,
        _lib.raw_stream(gy.device.index)), 'gconv3x3_grad_input')
    calls['grad_input'] += 1
    return gx


def grad_weight(gy, x, weight, stride):
    B, C, H, W = x.shape
    cpg = weight.shape[1]
    key = (B, C, cpg, H, W, stride)
    n = _sizes.get(key)
    if n is None:
        n = _sizes[key] = library().kgdet_gconv3x3_workspace_bytes(*key)
    ws = torch.empty(n, dtype=torch.uint8, device=x.device)
    gw = torch.empty_like(weight)
    _lib.check(library().kgdet_gconv3x3_grad_weight(
        gy.data_ptr(), x.data_ptr(), gw.data_ptr(), B, C, cpg, H, W, stride, ws.data_ptr(), n,
        _lib.raw_stream(x.device.index)), 'gconv3x3_grad_weight')
    calls['grad_weight'] += 1
    return gw


class _GroupedConv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, stride):
        weight = weight.contiguous()
        ctx.stride = stride
        ctx.save_for_backward(x, weight)
        return forward(x, weight, stride)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous()
        gx = grad_input(gy, weight, x.shape, ctx.stride) if ctx.needs_input_grad[0] else None
        gw = grad_weight(gy, x, weight, ctx.stride) if ctx.needs_input_grad[1] else None
        return gx, gw, None


def conv3x3(x, weight, stride=1):
    """the grouped convolution of an x that `applicable` accepted (a missing kernel or a refused shape raises)"""
    return _GroupedConv3x3.apply(x, weight, int(stride))


def conv3x3_bias_act(x, weight, bias, stride=1, relu=False):
    """inference: ``[relu](conv(x, weight) + bias[c])`` in the convolution's store (no autograd)"""
    return forward(x, weight.contiguous(), int(stride), bias.contiguous() if bias is not None else None, relu)
