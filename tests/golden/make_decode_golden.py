"""Generate tests/golden/decode_golden.npz: what ``get_bboxes(..., nms=False)`` of the KGDet head and of the serial head
returns for fabricated final-stage maps -- the decode arithmetic alone (top-k cut, stride / centre, clamps, rescale), recorded
at one commit so that a later commit can be held to it bit for bit (tests/test_decode.py).

B = 3 images of different ``img_shape`` / ``scale_factor``; two levels, 16 x 20 (stride 8) and 8 x 10 (stride 16);
``nms_pre`` = 50, so both levels are cut; maps are ``randn * 3`` so that boxes and landmarks leave every image and each clamp
rule acts.  Per case and image: boxes and scores in full, landmarks 0-5 and the last three (all residues mod 3: the serial
head clamps over the landmark axis) and the landmark tensor's shape.  Only the public ``get_bboxes`` is used, so the script
runs unchanged at any commit.  One recording per device; the file keeps those it is not asked to remake:

    python tests/golden/make_decode_golden.py --device cpu  --commit <hash>
    python tests/golden/make_decode_golden.py --device cuda --commit <hash>
"""
import argparse
import contextlib
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from kgdet_amd import configs  # noqa: E402
from kgdet_amd.registry import build_head  # noqa: E402
from tests import cpu_ops  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'decode_golden.npz')
LEVELS = ((16, 20), (8, 10))
STRIDES = [8, 16]
NMS_PRE = 50
IMG_SHAPES = ((128, 160, 3), (100, 150, 3), (120, 140, 3))
SCALE_FACTORS = (1.0, 1.5, 0.75)
PER_AXIS = ((1.0, 1.25, 1.0, 1.25), (1.5, 1.5, 1.5, 1.5), (0.75, 0.5, 0.75, 0.5))      # (w, h, w, h) per image
NP_FACTORS = tuple(np.float32(f) for f in SCALE_FACTORS)
K = 294
KPT_KEEP = [0, 1, 2, 3, 4, 5, K - 3, K - 2, K - 1]
#            name             head      rescale  scale factors   sigmoid
CASES = (('kgdet_rescale',    'kgdet',  True,    SCALE_FACTORS,  True),
         ('kgdet_plain',      'kgdet',  False,   SCALE_FACTORS,  True),
         ('serial_rescale',   'serial', True,    SCALE_FACTORS,  True),
         ('serial_plain',     'serial', False,   SCALE_FACTORS,  True),
         ('kgdet_np_factor',  'kgdet',  True,    NP_FACTORS,     True),     # not a python number: new_tensor(), true division
         ('kgdet_per_axis',   'kgdet',  True,    PER_AXIS,       True),     # raises: [n, K, 2] landmarks / a 4-vector
         ('kgdet_softmax',    'kgdet',  True,    SCALE_FACTORS,  False))


def build(kind, sigmoid):
    """a narrow head of either family: the decode reads its strides, class count and moment parameters, never its convolutions"""
    torch.manual_seed(0)
    cfg = (configs.kgdet_r50_fpn() if kind == 'kgdet' else configs.reppoints_kp_r50_fpn()).model.bbox_head.copy()
    cfg.update(in_channels=16, feat_channels=16, point_feat_channels=16, point_strides=list(STRIDES),
               norm_cfg=dict(type='GN', num_groups=4, requires_grad=True))
    head = build_head(cfg).eval()
    if not sigmoid:     # what a `loss_cls` dict without `use_sigmoid` sets (FocalLoss itself refuses to be built that way)
        head.use_sigmoid_cls, head.cls_out_channels = False, head.num_classes
    assert head.num_keypts == K
    return head


def maps(head, kind, device):
    """the arguments of ``get_bboxes`` in front of ``img_metas``: fabricated final-stage maps, the same for every device"""
    g = torch.Generator().manual_seed(0)
    draw = lambda c, hw: (torch.randn(3, c, *hw, generator=g) * 3).to(device)
    cls = [draw(head.cls_out_channels, hw) for hw in LEVELS]
    kpt = [draw(2 * K, hw) for hw in LEVELS]
    if kind == 'kgdet':
        return (None, None, cls, None, None, kpt, None, None, [draw(4, hw) for hw in LEVELS])
    return (cls, None, kpt, None, [draw(2 * head.num_reppts, hw) for hw in LEVELS])


def check_cut(head, cls, sigmoid):
    """a score may differ in its last bit between two commits (CPU sigmoid: vector lanes or scalar tail, by tensor shape); that
    must neither select nor order differently.  Around each level's cut (two ranks either side) neighbouring ranked maxima lie
    more than 1e-6 apart; among the kept ones more than two float32 ulps of a value below 1 (2 * 5.96e-8: both may move)"""
    for c in cls:
        s = c.permute(0, 2, 3, 1).reshape(c.shape[0], -1, c.shape[1]).double()
        m = (s.sigmoid() if sigmoid else s.softmax(-1)[..., 1:]).max(-1)[0]
        assert m.shape[1] > NMS_PRE + 2
        top = m.sort(dim=1, descending=True)[0][:, :NMS_PRE + 3]
        gaps = top[:, :-1] - top[:, 1:]                          # gaps[:, r]: rank r to rank r + 1; the cut is gap NMS_PRE - 1
        assert float(gaps[:, NMS_PRE - 3:NMS_PRE + 2].min()) > 1e-6, 'ranked maxima around the cut closer than 1e-6'
        assert float(gaps[:, :NMS_PRE].min()) > 1.2e-7, 'kept maxima closer than two ulps'


def run_case(name, device):
    """-> {'<name>:<image>:bboxes' | 'scores' | 'kpts' | 'kpts_shape': array}, or {'<name>:raises': True}"""
    _, kind, rescale, factors, sigmoid = next(c for c in CASES if c[0] == name)
    head = build(kind, sigmoid).to(device)
    args = maps(head, kind, device)
    check_cut(head, args[2] if kind == 'kgdet' else args[0], sigmoid)
    metas = [dict(img_shape=s, pad_shape=(128, 160, 3), scale_factor=f) for s, f in zip(IMG_SHAPES, factors)]
    cfg = (configs.kgdet_r50_fpn() if kind == 'kgdet' else configs.reppoints_kp_r50_fpn()).test_cfg.copy()
    cfg['nms_pre'] = NMS_PRE
    patch = cpu_ops.patched() if str(device) == 'cpu' else contextlib.nullcontext()     # (points2bbox of the serial head)
    with patch, torch.no_grad():
        try:
            res = head.get_bboxes(*args, metas, cfg, rescale=rescale, nms=False)
        except RuntimeError:        # recorded as such: the per-axis factor does not broadcast against the landmarks' (x, y)
            if factors is not PER_AXIS:
                raise
            return {name + ':raises': np.array(True)}
    out = {}
    for i, (bboxes, scores, kpts) in enumerate(res):
        out['%s:%d:bboxes' % (name, i)] = bboxes.cpu().numpy()
        out['%s:%d:scores' % (name, i)] = scores.cpu().numpy()
        out['%s:%d:kpts' % (name, i)] = kpts.reshape(kpts.shape[0], K, 3)[:, KPT_KEEP].cpu().numpy()
        out['%s:%d:kpts_shape' % (name, i)] = np.array(kpts.shape, dtype=np.int64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--device', required=True, choices=['cpu', 'cuda'])
    ap.add_argument('--commit', default=None, help='hash of the commit the recording is made at (default: git HEAD)')
    ap.add_argument('--out', default=PATH)
    a = ap.parse_args()
    commit = a.commit or subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=ROOT).decode().strip()
    data = dict(np.load(a.out)) if os.path.exists(a.out) else {}
    data = {k: v for k, v in data.items() if not k.startswith(a.device + ':')}
    data['commit:' + a.device] = np.array(commit)
    for case in CASES:
        for k, v in run_case(case[0], a.device).items():
            data['%s:%s' % (a.device, k)] = v
    np.savez_compressed(a.out, **data)
    print('wrote', a.out, os.path.getsize(a.out), 'bytes,', len(data), 'arrays, commit', commit)


if __name__ == '__main__':
    main()
