"""Generate tests/golden/resnext_golden.npz from the reference's ResNeXt, imported in place (needs a reference checkout; runs on
the CPU):

    python tests/golden/make_resnext_golden.py

Stored -- outputs and names only, every weight is rebuilt by the test from tests/resnext_cases.py's formulas:
  names:small / shapes:small, names:full / shapes:full   the ordered state-dict names and shapes of the small net
        (tests/resnext_cases.SMALL) and of ResNeXt-101 32x4d
  out64:<style>:<i>      the outputs of the small net in float64 on the formula input, style 'pytorch' and 'caffe'
  err32:<style>:<i>      max |float32 run - float64 run| / max |float64 run| of the reference's own float32 module
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import resnext_cases as X  # noqa: E402
from tests.golden import ref_loader  # noqa: E402


def _names(module):
    sd = module.state_dict()
    names = np.array(list(sd.keys()))
    shapes = np.zeros((len(sd), 4), np.int64)
    for i, t in enumerate(sd.values()):
        shapes[i, :t.dim()] = list(t.shape)
    return names, shapes


def main():
    ref_loader.load_detector()
    import importlib
    ResNeXt = importlib.import_module('mmdet.models.backbones.resnext').ResNeXt
    out = {}
    for style in X.STYLES:
        net = X.fill(ResNeXt(style=style, **X.SMALL))
        net.eval()
        if style == X.STYLES[0]:
            out['names:small'], out['shapes:small'] = _names(net)
        with torch.no_grad():
            y32 = net(X.formula_input(dtype=torch.float32))
            y64 = X.fill(net.double())(X.formula_input())
        for i, (a, b) in enumerate(zip(y32, y64)):
            out['out64:%s:%d' % (style, i)] = b.numpy()
            out['err32:%s:%d' % (style, i)] = np.float64((a.double() - b).abs().max() / b.abs().max())
    out['names:full'], out['shapes:full'] = _names(ResNeXt(**X.FULL))
    path = os.path.join(HERE, 'resnext_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', {k: float(v) for k, v in out.items() if k.startswith('err32')})


if __name__ == '__main__':
    main()
