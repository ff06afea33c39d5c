"""The small ResNeXt of the backbone tests: its keywords, the closed formulas that fill every parameter and buffer from its name
and index (no RNG: tests/golden/make_resnext_golden.py fills the reference's module, the tests fill this build's, with the same
numbers) and the formula input.  Plain CPU torch."""
import zlib

import torch

SMALL = dict(depth=50, groups=8, base_width=4, num_stages=2, strides=(1, 2), dilations=(1, 1), out_indices=(0, 1),
             frozen_stages=1)
FULL = dict(depth=101, groups=32, base_width=4)
STYLES = ('pytorch', 'caffe')
INPUT_SHAPE = (1, 3, 32, 48)


def _phase(name):
    return (zlib.crc32(name.encode()) % 6283) / 1000.0


def formula(name, shape, dtype=torch.float64):
    """the value of the state-dict entry ``name``: convolution weights are sines of amplitude 1.5 / sqrt(fan_in), BatchNorm
    scales 0.5 + cos(.) (negatives among them), shifts and means small sines, variances 1 + 0.5 sin(.) in [0.5, 1.5]"""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.float64)
    p = _phase(name)
    leaf = name.rsplit('.', 1)[-1]
    if leaf == 'num_batches_tracked':
        return torch.zeros(shape, dtype=torch.long)
    if len(shape) == 4:
        fan_in = shape[1] * shape[2] * shape[3]
        v = 1.5 / fan_in ** 0.5 * torch.sin(p + 0.7 * i + 0.013 * (i % 97) ** 2)
    elif leaf == 'weight':
        v = 0.5 + torch.cos(p + 1.3 * i)
    elif leaf == 'bias':
        v = 0.2 * torch.sin(p + 0.9 * i)
    elif leaf == 'running_mean':
        v = 0.1 * torch.sin(p + 0.5 * i)
    elif leaf == 'running_var':
        v = 1.0 + 0.5 * torch.sin(p + 1.1 * i)
    else:
        raise KeyError(name)
    return v.reshape(shape).to(dtype)


def fill(module):
    """every parameter and buffer of ``module`` from `formula`, in the module's own dtype"""
    with torch.no_grad():
        for name, t in module.state_dict().items():
            t.copy_(formula(name, tuple(t.shape)).to(t.dtype))
    return module


def formula_input(shape=INPUT_SHAPE, dtype=torch.float64):
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.float64)
    return (torch.sin(0.11 * i) + 0.5 * torch.cos(0.023 * i + 1.0)).reshape(shape).to(dtype)
