"""CPU tests of the host side: registry/config API, point grid, assigners, targets, losses, FPN2
pruning, head wiring (with the HIP ops replaced by test-side CPU references), checkpoint keys."""
import os
import re

import numpy as np
import pytest
import torch

import kgdet_amd
from kgdet_amd import configs, points, synthetic
from kgdet_amd.registry import (HEADS, Config, ConfigDict, Registry, build_detector, build_from_cfg, build_head)
from tests import cpu_ops

REF_CFG = '/root/reference/configs/kgdet_moment_r50_fpn_1x-demo.py'
REF_CONFIGS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_configs_golden.txt')


def _reference_config(name):
    """The reference's configs/<name>.py as Config.fromfile evaluates it.  Its model / train_cfg / test_cfg are recorded in
    tests/golden/ref_configs_golden.txt (tests/golden/make_config_golden.py); where the reference checkout is mounted the
    file itself is loaded and must equal the record."""
    import ast
    with open(REF_CONFIGS) as f:
        rec = Config(ast.literal_eval(f.read())[name])
    path = os.path.join(os.path.dirname(REF_CFG), name + '.py')
    if not os.path.isfile(path):
        return rec
    cfg = Config.fromfile(path)
    for k in ('model', 'train_cfg', 'test_cfg'):
        assert cfg[k] == rec[k], (name, k)
    return cfg


# ---- registry / config --------------------------------------------------------------------------
def test_registry_contract():
    R = Registry('thing')

    @R.register_module
    class A(object):
        def __init__(self, x, y=2):
            self.x, self.y = x, y

    assert R.get('A') is A and R.get('B') is None
    with pytest.raises(KeyError):
        R.register_module(A)                       # duplicate name
    with pytest.raises(TypeError):
        R._register_module(lambda: 0)
    obj = build_from_cfg(dict(type='A', x=1), R, default_args=dict(y=5, x=9))
    assert (obj.x, obj.y) == (1, 5)                # default_args only fill missing keys
    with pytest.raises(KeyError):
        build_from_cfg(dict(type='Nope'), R)
    with pytest.raises(AssertionError):
        build_from_cfg(dict(x=1), R)
    assert build_from_cfg(dict(type=A, x=3), R).x == 3


def test_registered_names_the_configs_need():
    for name in ('RepPointsHeadKp3RepCas1AssignOnce', 'KGDetHead'):
        assert HEADS.get(name) is kgdet_amd.heads.RepPointsHeadKp3RepCas1AssignOnce
    assert kgdet_amd.DETECTORS.get('RepPointsDetectorKp') is not None
    assert kgdet_amd.BACKBONES.get('ResNet') is not None
    assert kgdet_amd.NECKS.get('FPN2') is not None and kgdet_amd.NECKS.get('FPN') is not None
    assert kgdet_amd.LOSSES.get('FocalLoss') is not None and kgdet_amd.LOSSES.get('SmoothL1Loss') is not None


def test_config_dict_access(tmp_path):
    p = tmp_path / 'cfg.py'
    p.write_text("a = dict(b=dict(c=[1, dict(d=2)]), e=3)\nimport os\nf = 'x'\n")
    cfg = Config.fromfile(str(p))
    assert cfg.a.b.c[1].d == 2 and cfg.a['e'] == 3 and cfg.f == 'x'
    assert cfg.get('zzz', 7) == 7 and 'os' not in cfg
    assert cfg.a.get('nms_pre', -1) == -1
    with pytest.raises(FileNotFoundError):
        Config.fromfile(str(tmp_path / 'missing.py'))
    with pytest.raises(IOError):
        (tmp_path / 'c.yaml').write_text('a: 1')
        Config.fromfile(str(tmp_path / 'c.yaml'))


def test_reference_configs_load_unchanged():
    cfg = _reference_config('kgdet_moment_r50_fpn_1x-demo')
    mine = configs.kgdet_r50_fpn()
    assert cfg.model == mine.model and cfg.train_cfg == mine.train_cfg and cfg.test_cfg == mine.test_cfg
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    n = sum(p.numel() for p in model.parameters() if p.requires_grad)
    assert n == 59134423
    full = _reference_config('kgdet_moment_r50_fpn_1x-deepfashion2')
    assert full.model == mine.model


@pytest.mark.parametrize('name,parallel', [('serial', False), ('parallel', True)])
def test_reference_serial_parallel_configs_load_unchanged(name, parallel):
    cfg = _reference_config('reppoints_moment_%s_r50_fpn_1x-deepfashion2' % name)
    mine = configs.reppoints_kp_r50_fpn(parallel=parallel)
    assert cfg.model == mine.model and cfg.train_cfg == mine.train_cfg and cfg.test_cfg == mine.test_cfg
    head = build_head(cfg.model.bbox_head)
    keys = set(head.state_dict().keys())
    assert {'cls_refine_dfmconv.weight', 'keypts_init_conv.weight', 'reppts_init_out.bias',
            'keypts_refine_dfmconv.weight', 'reppts_refine_out.weight', 'moment_transfer'} <= keys
    assert ('reppts_refine_dfmconv.weight' in keys) == parallel and ('reppts_init_conv.weight' in keys) == parallel
    assert tuple(head.reppts_init_out.weight.shape) == ((18, 256, 1, 1) if parallel else (18, 588, 1, 1))


@pytest.mark.parametrize('parallel', [False, True])
def test_serial_parallel_head_forward_loss_decode_on_cpu(parallel):
    torch.manual_seed(0)
    cfg = configs.reppoints_kp_r50_fpn(parallel=parallel)
    hc = cfg.model.bbox_head.copy()
    hc.update(in_channels=16, feat_channels=16, point_feat_channels=16, point_strides=[8, 16],
              norm_cfg=dict(type='GN', num_groups=4, requires_grad=True))
    head = build_head(hc)
    head.init_weights()
    feats = [torch.randn(2, 16, 16, 20), torch.randn(2, 16, 8, 10)]
    batch = synthetic.make_batch(2, 'cpu', seed=2, img_shape=(128, 160, 3), pad_shape=(128, 160, 3))
    for k in ('gt_bboxes', 'gt_keypoints'):
        batch[k] = [t.clamp(max=120) for t in batch[k]]
    with cpu_ops.patched():
        outs = head(feats, batch['img_meta'])
        assert len(outs) == 5 and outs[0][0].shape == (2, 13, 16, 20) and outs[3][1].shape == (2, 18, 8, 10)
        losses = head.loss(*outs, batch['gt_bboxes'], batch['gt_labels'], batch['gt_keypoints'], batch['img_meta'],
                           cfg.train_cfg)
        assert sorted(losses) == ['loss_bbox_init', 'loss_bbox_refine', 'loss_cls', 'loss_kpt_init', 'loss_kpt_refine']
        total = sum(sum(v) for v in losses.values())
        assert torch.isfinite(total)
        total.backward()
        assert head.cls_refine_dfmconv.weight.grad.abs().sum() > 0
        head.eval()
        with torch.no_grad():
            res = head.get_bboxes(*head(feats, batch['img_meta']), batch['img_meta'], cfg.test_cfg, rescale=True,
                                  nms=False)
    assert res[0][0].shape == (400, 4) and res[0][1].shape == (400, 14) and res[0][2].shape == (400, 882)


def test_checkpoint_key_contract():
    cfg = configs.kgdet_r50_fpn()
    head = build_head(cfg.model.bbox_head)
    keys = set(head.state_dict().keys())
    for k in ('cls_convs.0.conv.weight', 'cls_convs.2.gn.bias', 'reg_convs.1.gn.weight', 'moment_transfer',
              'kp_rep_block_1.cls_conv.weight', 'kp_rep_block_1.keypts_out.bias',
              'kp_rep_block_2.cls_dfmconv_3.weight', 'kp_rep_block_3.keypts_dfmconv_7.weight',
              'kp_rep_block_3.reppts_out.weight', 'kp_rep_block_2.cls_out.bias'):
        assert k in keys, k
    assert not any('dcn_base_offset' in k for k in keys)       # plain attributes, not buffers (KP3:47)
    assert head.num_reppts == 83 and head.cls_out_channels == 13
    assert tuple(head.kp_rep_block_2.cls_dfmconv_7.weight.shape) == (256, 256, 7, 7)
    assert tuple(head.kp_rep_block_2.reppts_out.weight.shape) == (166, 588, 1, 1)


# ---- point grid / assigners / targets ----------------------------------------------------------
def test_point_generator():
    g = points.PointGenerator()
    p = g.grid_points((2, 3), 32, device='cpu')
    assert p.tolist() == [[0, 0, 32], [32, 0, 32], [64, 0, 32], [0, 32, 32], [32, 32, 32], [64, 32, 32]]
    f = g.valid_flags((2, 3), (1, 2), device='cpu')
    assert f.tolist() == [True, True, False, False, False, False]


def _grid(h=25, w=42, stride=32):
    return points.PointGenerator().grid_points((h, w), stride, device='cpu')


def test_point_assigner_single_gt_takes_k_nearest():
    pts = _grid()
    gt = torch.tensor([[320., 160., 640., 480.]])              # centre (480, 320) = grid cell (15, 10)
    res = points.PointAssigner(scale=4, pos_num=9).assign(pts, gt, None, torch.tensor([5]))
    pos = torch.nonzero(res.gt_inds > 0).flatten().tolist()
    expect = sorted((10 + dy) * 42 + (15 + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    assert pos == expect and set(res.labels[pos].tolist()) == {5}
    assert int((res.gt_inds == 0).sum()) == 1050 - 9
    with pytest.raises(ValueError):
        points.PointAssigner().assign(pts, gt[:0])


def test_point_assigner_overlapping_gts_nearest_wins():
    pts = _grid()
    gts = torch.tensor([[320., 160., 640., 480.], [352., 160., 672., 480.]])   # centres one cell apart
    res = points.PointAssigner(scale=4, pos_num=9).assign(pts, gts, None, torch.tensor([1, 2]))
    inds = res.gt_inds.view(25, 42)
    assert inds[10, 14] == 1 and inds[10, 17] == 2               # exclusive columns
    assert inds[10, 15] == 1 and inds[10, 16] == 2               # shared cells go to the nearer centre
    assert int((res.gt_inds > 0).sum()) == 12


def test_point_target_kp_shapes_and_counts():
    batch = synthetic.make_batch(2, 'cpu', seed=3)
    gen = points.PointGenerator()
    centers = [[gen.grid_points((25, 42), 32, device='cpu')] for _ in range(2)]
    flags = [[gen.valid_flags((25, 42), (25, 42), device='cpu')] for _ in range(2)]
    cfg = ConfigDict(assigner=dict(type='PointAssigner', scale=4, pos_num=25), allowed_border=-1, pos_weight=-1,
                     debug=False)
    out = points.point_target_kp(centers, flags, batch['gt_bboxes'], batch['gt_keypoints'], batch['img_meta'], cfg,
                                 gt_labels_list=batch['gt_labels'], label_channels=13, sampling=False)
    labels, lw, bbox_gt, _, bw, kgt, kw, n_pos, n_neg = out
    assert labels[0].shape == (2, 1050) and kgt[0].shape == (2, 1050, 294, 2)
    assert n_pos == int((labels[0] > 0).sum()) and 25 <= n_pos <= 100
    assert torch.all(lw[0] == 1) and torch.all(bw[0][labels[0] > 0] == 1)
    # keypoint weights mark exactly the visible keypoints of the assigned GT's category slice
    b, i = torch.nonzero(labels[0] > 0)[0].tolist()
    lo, hi = synthetic.CLASS_KEYPOINT_SLICES[int(labels[0][b, i])]
    assert kw[0][b, i, lo:hi].min() == 1 and kw[0][b, i].sum() == 2 * (hi - lo)


def test_max_iou_assigner():
    a = points.MaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0)
    boxes = torch.tensor([[0., 0., 9., 9.], [0., 0., 9., 4.], [50., 50., 60., 60.], [0., 0., 9., 7.]])
    res = a.assign(boxes, torch.tensor([[0., 0., 9., 9.]]), None, torch.tensor([3]))
    assert res.gt_inds.tolist() == [1, 1, 0, 1] and res.labels.tolist() == [3, 3, 0, 3]
    iou = points.bbox_overlaps(torch.tensor([[0., 0., 9., 9.]]), boxes)
    np.testing.assert_allclose(iou.numpy(), [[1.0, 0.5, 0.0, 0.8]], rtol=1e-6)


# ---- losses ------------------------------------------------------------------------------------
def test_smooth_l1_and_reduction():
    from kgdet_amd.losses import SmoothL1Loss, weight_reduce_loss
    pred = torch.tensor([[0.0, 0.05, 1.0]])
    tgt = torch.zeros(1, 3)
    l = SmoothL1Loss(beta=1.0 / 9.0, loss_weight=0.5)(pred, tgt, torch.ones(1, 3), avg_factor=2.0)
    beta = 1.0 / 9.0
    expect = 0.5 * (0.5 * 0.05 ** 2 / beta + (1.0 - 0.5 * beta)) / 2.0
    assert abs(float(l) - expect) < 1e-7
    with pytest.raises(ValueError):
        weight_reduce_loss(torch.ones(3), None, 'sum', avg_factor=2)


# ---- neck --------------------------------------------------------------------------------------
def test_fpn2_pruned_forward_equals_full_pyramid():
    from kgdet_amd.neck import FPN, FPN2
    torch.manual_seed(0)
    kw = dict(in_channels=[8, 16, 32, 64], out_channels=32, num_outs=5, start_level=1, add_extra_convs=True,
              norm_cfg=dict(type='GN', num_groups=8, requires_grad=True))
    sel = FPN2(select_out=[2], **kw)
    full = FPN(**kw)
    full.load_state_dict(sel.state_dict())
    feats = [torch.randn(2, c, 64 // s, 80 // s) for c, s in zip([8, 16, 32, 64], [1, 2, 4, 8])]
    out = sel(feats)
    assert len(out) == 1 and torch.equal(out[0], full(feats)[2])
    out[0].sum().backward()
    dead = [n for n, p in sel.named_parameters() if p.grad is None]
    live = [n for n, p in sel.named_parameters() if p.grad is not None]
    assert all(n.startswith(('lateral_convs.2', 'fpn_convs.2')) for n in live) and len(dead) > 0


# ---- head wiring on CPU (HIP ops replaced by the test references) -------------------------------
def _small_head():
    torch.manual_seed(0)
    cfg = configs.kgdet_r50_fpn().model.bbox_head.copy()
    cfg.update(in_channels=32, feat_channels=32, point_feat_channels=32, num_keypts=294,
               norm_cfg=dict(type='GN', num_groups=8, requires_grad=True))
    head = build_head(cfg)
    head.init_weights()
    return head


def test_head_forward_loss_and_decode_on_cpu():
    head = _small_head()
    x = torch.randn(2, 32, 8, 10)
    batch = synthetic.make_batch(2, 'cpu', seed=1, img_shape=(256, 320, 3), pad_shape=(256, 320, 3))
    for k in ('gt_bboxes', 'gt_keypoints'):
        batch[k] = [t.clamp(max=250) for t in batch[k]]
    with cpu_ops.patched():
        outs = head([x], batch['img_meta'])
        assert len(outs) == 9 and outs[0][0].shape == (2, 13, 8, 10)
        assert outs[3][0].shape == (2, 588, 8, 10) and outs[6][0].shape == (2, 4, 8, 10)
        tcfg = configs.kgdet_r50_fpn().train_cfg
        losses = head.loss(*outs, batch['gt_bboxes'], batch['gt_labels'], batch['gt_keypoints'], batch['img_meta'],
                           tcfg)
        assert sorted(losses) == sorted(['loss_%s_%d' % (n, s) for n in ('cls', 'bbox', 'kpt') for s in (1, 2, 3)])
        total = sum(sum(v) for v in losses.values())
        assert torch.isfinite(total)
        total.backward()
        assert head.kp_rep_block_3.cls_dfmconv_5.weight.grad.abs().sum() > 0
        assert head.moment_transfer.grad.abs().sum() > 0
        # stage-1 outputs only reach later stages detached: their reppts conv sees gradient from the
        # stage-1 bbox loss and (scaled by gradient_mul) from the stage-2 offsets
        assert head.kp_rep_block_1.reppts_out.weight.grad.abs().sum() > 0
    # decode path without NMS (pure torch) keeps the reference's shapes and clamping
    head.eval()
    with cpu_ops.patched(), torch.no_grad():
        outs = head([x], batch['img_meta'])
        tst = configs.kgdet_r50_fpn().test_cfg
        res = head.get_bboxes(*outs, batch['img_meta'], tst, rescale=True, nms=False)
    bboxes, scores, kpts = res[0]
    assert bboxes.shape == (80, 4) and scores.shape == (80, 14) and kpts.shape == (80, 882)
    assert torch.all(scores[:, 0] == 0) and bboxes.max() <= 320 and bboxes.min() >= 0
    assert torch.all(kpts.view(80, 294, 3)[:, :, 2] == 1)


def test_points2kpt_and_offset_to_pts():
    head = _small_head()
    pts = torch.arange(2 * 6 * 2 * 3, dtype=torch.float32).view(2, 6, 2, 3)     # 3 points, (y, x) interleaved
    k = head.points2kpt(pts)
    assert torch.equal(k[:, 0::2], pts[:, 1::2]) and torch.equal(k[:, 1::2], pts[:, 0::2])
    head.point_strides = [32]
    centers = [[points.PointGenerator().grid_points((2, 3), 32, device='cpu')] for _ in range(2)]
    out = head.offset_to_pts(centers, [pts])[0]                                 # [B, HW, 2n] as x0,y0,x1,y1..
    b, hw, i = 1, 4, 2
    h, w = divmod(hw, 3)
    assert out[b, hw, 2 * i] == pts[b, 2 * i + 1, h, w] * 32 + centers[0][0][hw, 0]
    assert out[b, hw, 2 * i + 1] == pts[b, 2 * i, h, w] * 32 + centers[0][0][hw, 1]


# ---- C ABI -------------------------------------------------------------------------------------
def test_shared_library_exports_every_declared_symbol():
    import ctypes
    from kgdet_amd import _lib
    header = open(os.path.join(os.path.dirname(kgdet_amd.__file__), '..', 'include', 'kgdet_hip.h')).read()
    names = set(re.findall(r'\b(kgdet_[a-z0-9_]+)\s*\(', header))
    assert len(names) >= 20
    L = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in sorted(names) if not hasattr(L, n)]
    assert not missing, missing
    assert L.kgdet_version() == 1
    s = _lib.DcnShape(2, 256, 25, 42, 256, 7, 7, 1, 1, 3, 3, 1, 1, 1, 1, 0, 0)
    L.kgdet_dcn_packed_weight_bytes.restype = ctypes.c_size_t
    assert L.kgdet_dcn_packed_weight_bytes(ctypes.byref(s)) == 4 * 49 * 256 * 256 * 4  # fp32 fwd, fp32 bwd, bf16 hi/lo, its transpose
    bad = _lib.DcnShape(2, 256, 2, 2, 256, 7, 7, 1, 1, 0, 0, 1, 1, 1, 1, 0, 0)
    ho, wo = ctypes.c_int32(), ctypes.c_int32()
    assert L.kgdet_dcn_output_size(ctypes.byref(bad), ctypes.byref(ho), ctypes.byref(wo)) == _lib.KGDET_E_SHAPE
    L.kgdet_last_error.restype = ctypes.c_char_p
    assert b'too small' in L.kgdet_last_error()


def test_group_norm_slice_count_never_returns_to_one_workgroup_for_large_groups():
    """a group beyond the one-workgroup kernels' 65536 elements keeps at least two slices however many
    (image, group) pairs there are (batch 32 x 32 groups at 100 x 168 used to get S = 1 and then a shape error)"""
    import ctypes
    from kgdet_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.kgdet_gn_act_slices.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]
    L.kgdet_gn_act_slices.restype = ctypes.c_int32
    assert L.kgdet_gn_act_slices(2, 256, 32, 25 * 42) == 1                  # 8 x 1050 elements: one workgroup
    for n in (1, 2, 8, 31, 32, 64, 1000):
        s = L.kgdet_gn_act_slices(n, 256, 32, 100 * 168)                   # 8 x 16800 = 134400 elements per group
        assert 2 <= s <= 16, (n, s)
    assert L.kgdet_gn_act_slices(4096, 64, 1, 200 * 336) >= 2


def test_ops_have_no_cpu_fallback():
    from kgdet_amd import dcn, focal_loss, moment
    with pytest.raises(NotImplementedError):
        dcn.deform_conv(torch.zeros(1, 4, 5, 5), torch.zeros(1, 18, 5, 5), torch.zeros(4, 4, 3, 3), 1, 1, 1)
    with pytest.raises(NotImplementedError):
        moment.moment_bbox(torch.zeros(1, 18, 2, 2), torch.zeros(2))
    with pytest.raises(NotImplementedError):
        focal_loss.sigmoid_focal_loss(torch.zeros(2, 3), torch.zeros(2, dtype=torch.long), 2.0, 0.25)


def test_dense_targets_equal_mirrored_path():
    """point_target_kp_dense (no host syncs) == the reference-mirroring point_target_kp on a single level:
    overlapping GTs, a GT with no visible keypoints, ties in the point-to-centre distance."""
    from kgdet_amd import points as P
    from kgdet_amd.registry import ConfigDict
    cfg = ConfigDict(assigner=dict(type='PointAssigner', scale=4, pos_num=25), allowed_border=-1, pos_weight=-1,
                     debug=False)
    gen = P.PointGenerator()
    g = torch.Generator().manual_seed(3)
    for trial in range(4):
        pts = gen.grid_points((25, 42), 32, device='cpu')
        n_gt = 1 + trial
        xy = torch.rand(n_gt, 2, generator=g) * torch.tensor([900., 500.]) + 100
        wh = torch.rand(n_gt, 2, generator=g) * 500 + 150
        if trial == 1:
            xy[0] = torch.tensor([16 * 32. + 16, 10 * 32. + 16])      # centre equidistant from 4 grid points
        if trial >= 2:
            xy[1] = xy[0] + 40                                        # overlapping GTs compete for points
        gt_b = torch.cat([xy - wh / 2, xy + wh / 2], 1)
        gt_l = torch.randint(1, 14, (n_gt, ), generator=g)
        gt_k = torch.rand(n_gt, 294, 3, generator=g) * 800
        gt_k[:, :, 2] = (torch.rand(n_gt, 294, generator=g) > 0.7).float() * 2
        if trial == 3:
            gt_k[0, :, 2] = 0
        metas = [dict(pad_shape=(800, 1344, 3), img_shape=(800, 1333, 3))] * 2
        props = [[pts.clone()], [pts.clone()]]
        valid = [[torch.ones(pts.shape[0], dtype=torch.uint8)], [torch.ones(pts.shape[0], dtype=torch.uint8)]]
        gtb, gtk, gtl = [gt_b, gt_b.flip(0)], [gt_k, gt_k.flip(0)], [gt_l, gt_l.flip(0)]
        ref = P.point_target_kp([list(p) for p in props], valid, gtb, gtk, metas, cfg, gt_labels_list=gtl,
                                label_channels=13, sampling=False)
        new = P.point_target_kp_dense([list(p) for p in props], gtb, gtk, cfg, gt_labels_list=gtl)
        assert P.dense_targets_applicable(cfg, 1, True, None)
        for a, b in zip(ref[:7], new[:7]):
            assert len(a) == len(b) == 1
            assert a[0].shape == b[0].shape and a[0].dtype == b[0].dtype
            assert torch.equal(a[0], b[0])
        assert int(new[7]) == ref[7] and int(new[8]) == ref[8]


def test_inference_bn_fold_matches_unfolded_backbone():
    """conv_bn folds frozen BatchNorm statistics into the convolution when autograd is off; same features"""
    from kgdet_amd.backbone import ResNet
    torch.manual_seed(0)
    m = ResNet(depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1, style='pytorch')
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.1)
    m.eval()
    x = torch.randn(1, 3, 64, 96)
    with torch.enable_grad():
        ref = m(x)            # unfolded: bn(conv(x))
    with torch.no_grad():
        out = m(x)            # folded
        m.layer2[0].conv1.weight.mul_(2.0)
        m.train()
        m.eval()              # mode switch drops the folded weights
        out2 = m(x)
    for a, b in zip(ref, out):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5 * float(a.abs().max()))
    assert not torch.allclose(out[1], out2[1])


def test_no_reference_text_in_tree():
    """Round-2 review item 2: nothing derived from the reference's sources lives in the working tree (which is what
    `gpurun` snapshots to the GPU box).  The reference build (oracle/build_ref.py) writes to $KGDET_REF_BUILD outside
    the tree; Cython-generated C embeds the .pyx text, so any generated C / oracle/_ref directory is a failure, and
    where the reference is mounted the distinctive lines of soft_nms_cpu.pyx / nms_cpu.cpp are searched for."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert not os.path.exists(os.path.join(root, 'oracle', '_ref'))
    from oracle import build_ref
    assert not os.path.abspath(build_ref.OUT).startswith(root + os.sep)
    needles = []
    src_dir = '/root/reference/mmdetection/mmdet/ops/nms/src'
    for name in ('soft_nms_cpu.pyx', 'nms_cpu.cpp'):
        path = os.path.join(src_dir, name)
        if os.path.isfile(path):
            for line in open(path):
                t = ' '.join(line.split())
                if len(t) >= 40 and not t.startswith(('#', '//', '*')):
                    needles.append(t)
    skip_dirs = {'.git', 'gpurun_out', '__pycache__', '.pytest_cache', 'build', '.hypothesis'}
    for dirpath, dirnames, filenames in os.walk(root):
        dirnames[:] = [d for d in dirnames if d not in skip_dirs and not d.startswith('build_')]
        for fn in filenames:
            if fn.endswith(('.so', '.o', '.npz', '.pyc', '.png', '.jpg')):
                continue
            path = os.path.join(dirpath, fn)
            if os.path.getsize(path) > 8 << 20:
                continue
            text = open(path, errors='ignore').read()
            assert 'Generated by ' + 'Cython' not in text, path
            if needles:
                flat = ' '.join(text.split())
                hits = [n for n in needles if n in flat]
                assert len(hits) < 3, (path, hits[:3])


def test_nms_workspace_bound_covers_every_split():
    """kgdet_nms_workspace_bytes is an upper bound of what nms_segments_large lays out (csrc/nms.hip: per segment
    roundup256(np * 8 + 24 n + roundup16(n)), np = max(64, next power of two >= n)) for any split -- the size query is
    host arithmetic, no GPU needed (the old bound was short for many tiny segments)."""
    import ctypes
    import numpy as np
    from kgdet_amd import _lib
    L = _lib.lib()

    def layout(lengths):
        tot = 16
        for n in lengths:
            npow = 64
            while npow < n:
                npow <<= 1
            tot += (npow * 8 + 24 * n + ((n + 15) & ~15) + 255) & ~255
        return tot
    rng = np.random.default_rng(0)
    cases = [[4100] + [0] * 999, [4100] + [1] * 999, [4097], [4097, 4097, 65], [12000, 64, 65, 0, 1],
             [5000] + [63] * 500 + [65] * 500]
    for _ in range(20):
        cases.append([int(rng.integers(4097, 20000))] + [int(v) for v in rng.integers(0, 200, size=int(rng.integers(0, 3000)))])
    for lengths in cases:
        need = layout(lengths)
        got = L.kgdet_nms_workspace_bytes(ctypes.c_int64(sum(lengths)), ctypes.c_int32(len(lengths)))
        assert got >= need, (lengths[:5], len(lengths), got, need)


def test_dcn_workspace_queries_are_consistent():
    """kgdet_dcn_workspace_bytes / kgdet_dcn_group_workspace_bytes / kgdet_dcn_packed_weight_bytes (csrc/dcn_api.hip) are host
    arithmetic: over N in {1, 2, 8}, the shapes of tests/dcn_edge_cases.py and the head's shapes (C = O = 256, 3x3 / 5x5 / 7x7, the
    five pyramid levels of an 800 x 1333 input, groups / deformable groups in {1, 2}) the group query covers every member's single
    query and grows with every problem added, a single query is positive exactly when kgdet_dcn_output_size accepts the shape, and
    the packed weight's size depends on the weight alone (the comment on split_images_ok: one pack serves every pyramid level and
    batch size)."""
    import ctypes
    from kgdet_amd import _lib
    from tests import dcn_edge_cases as E
    L = _lib.lib()

    def shape(N, C, H, W, O, k, s, p, d, g, dg):
        return _lib.DcnShape(N, C, H, W, O, k, k, s, s, p, p, d, d, g, dg, 0, 0)
    single = lambda s: L.kgdet_dcn_workspace_bytes(ctypes.byref(s))

    def group(shapes):
        arr = (ctypes.POINTER(_lib.DcnShape) * len(shapes))(*[ctypes.pointer(s) for s in shapes])
        return L.kgdet_dcn_group_workspace_bytes(len(shapes), arr)
    levels = [(-(-800 // st), -(-1344 // st)) for st in (8, 16, 32, 64, 128)]      # 800 x 1333 padded to a multiple of 32
    assert levels[0] == (100, 168) and levels[-1] == (7, 11)
    head = [(1, 256, H, W, 256, k, 1, k // 2, 1, g, dg) for H, W in levels for k in (3, 5, 7) for g in (1, 2) for dg in (1, 2)]
    packed = {}
    for N in (1, 2, 8):
        shapes = [shape(N, *c[1:]) for c in list(E.CASES) + head]
        for s in shapes:
            ok = L.kgdet_dcn_output_size(ctypes.byref(s), None, None) == _lib.KGDET_OK
            assert ok and single(s) > 0, ('a valid shape without a workspace size', N, s.C, s.H, s.W, s.kh)
            key = (s.C, s.O, s.kh, s.groups, s.deformable_groups)
            nbytes = L.kgdet_dcn_packed_weight_bytes(ctypes.byref(s))
            assert nbytes > 0 and packed.setdefault(key, nbytes) == nbytes, ('packed weight bytes depend on N, H or W', key, N, s.H, s.W)
        # the stages the head launches: per level, the kernel sizes of one (groups, deformable groups) choice on two maps
        stages = [[s for s in shapes[len(E.CASES):] if (s.H, s.groups, s.deformable_groups) == (H, g, dg)] * 2
                  for H, _ in levels for g in (1, 2) for dg in (1, 2)]
        stages += [shapes[:len(E.CASES)], [shape(N, 16, 6, 7, 16, k, 1, k // 2, 1, 1, 1) for k in (3, 5, 7)] * 2]
        for members in stages:
            assert len(members) >= 3
            prev = 0
            for n in range(1, len(members) + 1):
                got = group(members[:n])
                assert got >= max(single(s) for s in members[:n]), ('group query below a member\'s single query', N, n)
                assert got >= prev, ('group query shrinks when a problem is added', N, n, got, prev)
                prev = got
    # shapes kgdet_dcn_output_size refuses: no workspace size, no packed size, and a group that holds one has none either
    good = shape(2, 16, 6, 7, 16, 3, 1, 1, 1, 1, 1)
    for bad in (shape(2, 16, 1, 9, 16, 7, 1, 0, 1, 1, 1), shape(2, 16, 6, 7, 16, 3, 1, 1, 4, 1, 1), shape(0, 16, 6, 7, 16, 3, 1, 1, 1, 1, 1),
                shape(2, 16, 6, 7, 16, 3, 0, 1, 1, 1, 1), shape(2, 15, 6, 7, 16, 3, 1, 1, 1, 2, 1), shape(2, 16, 6, 7, 16, 3, 1, 1, 1, 1, 3)):
        assert L.kgdet_dcn_output_size(ctypes.byref(bad), None, None) != _lib.KGDET_OK
        assert single(bad) == 0 and L.kgdet_dcn_packed_weight_bytes(ctypes.byref(bad)) == 0 and group([good, bad]) == 0
    assert single(good) > 0


def _run_bench(argv, env_extra):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **env_extra)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        if k not in env_extra:
            env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(root, 'bench.py')] + argv, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=300)


def test_bench_refuses_an_n_gpu_line_from_fewer_devices():
    """`bench.py --gpus N` (reference: tools/dist_train.sh:8-10 starts the ranks) checks the device count BEFORE anything
    touches a GPU and exits non-zero with a message instead of printing an N-GPU line from fewer devices."""
    import torch
    n = torch.cuda.device_count() + 2
    r = _run_bench(['--gpus', str(n), '--steps', '1', '--warmup', '0'], {})
    assert r.returncode != 0
    assert b'refusing to print' in r.stderr and not any(l.startswith(b'{') for l in r.stdout.splitlines())


def test_bench_world_size_mismatch_exits_nonzero():
    """Launched by a torch.distributed.run whose --nproc-per-node differs from --gpus: exit, do not measure."""
    r = _run_bench(['--gpus', '4', '--steps', '1', '--warmup', '0'],
                   {'RANK': '0', 'LOCAL_RANK': '0', 'WORLD_SIZE': '2', 'MASTER_ADDR': '127.0.0.1', 'MASTER_PORT': '29999'})
    assert r.returncode != 0
    assert b'WORLD_SIZE=2' in r.stderr and not any(l.startswith(b'{') for l in r.stdout.splitlines())


def test_bench_rank0_block_never_steps_a_multi_rank_job_alone():
    """bench.py prints from rank 0 and measures a few extra legs there; a training step of an N-rank job contains collectives, so
    every `step()` (or `timed_window()`) call inside the `if rank == 0:` block must sit under a condition that says `world == 1`
    (round 5: the exact-fp32 leg was added without it and would have hung the N-rank scaling run)."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'bench.py')).read().splitlines()
    start = next(i for i, l in enumerate(src) if l.startswith('    if rank == 0:'))
    end = next(i for i in range(start + 1, len(src)) if src[i].strip() and len(src[i]) - len(src[i].lstrip()) <= 4)
    calls = 0
    for i in range(start + 1, end):
        line = src[i]
        code = line.split('#')[0]
        if 'step()' not in code and 'timed_window()' not in code:
            continue
        if code.lstrip().startswith(('def ', "'", '"')):
            continue
        calls += 1
        indent = len(line) - len(line.lstrip())
        guarded, j = False, i - 1
        while j > start:
            l = src[j]
            if l.strip():
                ind = len(l) - len(l.lstrip())
                if ind < indent:
                    indent = ind
                    if l.lstrip().startswith(('if ', 'elif ')) and 'world == 1' in l:
                        guarded = True
                        break
            j -= 1
        assert guarded, 'bench.py:%d calls a step inside the rank-0 block without a `world == 1` guard: %s' % (i + 1, line.strip())
    assert calls >= 1


def test_shared_levels_node_equals_per_level_graphs():
    """layers.shared_levels (config 5's head: the FPN levels of a shared-weight module as ONE autograd node whose backward sums the
    parameter gradients over the levels) == the plain per-level application (reppoints_head_kp_serial.py:495-497 multi_apply): outputs,
    input gradients and parameter gradients, including a parameter one level does not use and an output without gradient."""
    import torch
    import torch.nn as nn
    from kgdet_amd.layers import shared_levels

    class Head(nn.Module):
        def __init__(self):
            super().__init__()
            self.c = nn.Conv2d(3, 4, 3, padding=1)
            self.d = nn.Conv2d(4, 2, 1)
            self.only_small = nn.Parameter(torch.ones(1))

        def single(self, x):
            h = torch.relu(self.c(x))
            if x.shape[-1] <= 4:
                h = h * self.only_small
            return self.d(h), h.mean(1, keepdim=True).detach(), h.sum(1, keepdim=True) * 0.1

    torch.manual_seed(0)
    m = Head()
    xs = [torch.randn(2, 3, 8, 8, requires_grad=True), torch.randn(2, 3, 4, 4, requires_grad=True), torch.randn(1, 3, 6, 5)]
    outs = shared_levels(m, m.single, xs)
    assert len(outs) == 3 and all(len(o) == 3 for o in outs)
    sum(o.pow(2).sum() for j in (0, 2) for o in outs[j]).backward()
    got_p = [p.grad.clone() for p in m.parameters()]
    got_x = [x.grad.clone() for x in xs[:2]]
    for p in m.parameters():
        p.grad = None
    for x in xs[:2]:
        x.grad = None
    ref = [m.single(x) for x in xs]
    for j in range(3):
        for l in range(3):
            assert torch.equal(outs[j][l], ref[l][j])
    sum(r[j].pow(2).sum() for r in ref for j in (0, 2)).backward()
    for a, p in zip(got_p, m.parameters()):
        assert torch.allclose(a, p.grad, rtol=1e-6, atol=1e-7)
    for a, x in zip(got_x, xs[:2]):
        assert torch.allclose(a, x.grad, rtol=1e-6, atol=1e-7)
    assert xs[2].grad is None
