"""A static batch through the detector: ``forward_train`` on a loaded ``static_batch.StaticBatch`` -- ground truth in buffers of
fixed capacity, counts and valid extents in a device table read by the fused head-loss kernels -- against ``forward_train`` on
the same canvas tensor with plain lists.

The full-size KGDet detector on a small canvas: (256, 320) is a grid of 8 x 10 = 80 points at stride 32 with pos_num = 25; the
smallest pad_shape used is (192, 256), 48 valid points.  The comparison sees the SAME canvas tensor: a batch on a canvas is
that batch collated to a larger common size (static_batch), not the tight batch."""
import pytest
import torch

from kgdet_amd import runner as rn

pytestmark = pytest.mark.gpu

CANVAS = (256, 320)


def _make(config='kgdet'):
    from kgdet_amd import build_detector, configs
    from kgdet_amd.dist import DistOptimizerHook
    cfg = configs.kgdet_r50_fpn() if config == 'kgdet' else configs.reppoints_kp_r50_fpn(soft_nms=True)
    torch.manual_seed(0)
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda().train()
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-5)
    return model, opt, DistOptimizerHook(grad_clip=dict(max_norm=35, norm_type=2))


def _batch(counts, pads, seed, hw=None):
    """a host batch as ``datasets.collate`` makes it: ``img`` [B, 3, h, w] at the largest pad_shape (or ``hw``), zero beyond each
    image's own pad_shape; ``counts[b]`` garments inside image b"""
    from kgdet_amd import synthetic
    g = torch.Generator().manual_seed(seed)
    h, w = hw or (max(p[0] for p in pads), max(p[1] for p in pads))
    img = torch.randn(len(counts), 3, h, w, generator=g)
    out = dict(img=img, img_meta=[], gt_bboxes=[], gt_labels=[], gt_keypoints=[])
    for b, (n, pad) in enumerate(zip(counts, pads)):
        img[b, :, pad[0]:, :] = 0
        img[b, :, :, pad[1]:] = 0
        H, W = pad[0], pad[1] - 5
        out['img_meta'].append(synthetic.make_img_metas(1, (H, W, 3), (pad[0], pad[1], 3))[0])
        wh = torch.rand(n, 2, generator=g) * 110 + 40
        xy = torch.rand(n, 2, generator=g) * (torch.tensor([W - 1., H - 1.]) - wh)
        boxes = torch.cat([xy, xy + wh], 1)
        labels = torch.randint(1, 14, (n, ), generator=g)
        kps = torch.zeros(n, 294, 3)
        for i in range(n):
            lo, hi = synthetic.CLASS_KEYPOINT_SLICES[int(labels[i])]
            kps[i, lo:hi, 0] = boxes[i, 0] + torch.rand(hi - lo, generator=g) * wh[i, 0]
            kps[i, lo:hi, 1] = boxes[i, 1] + torch.rand(hi - lo, generator=g) * wh[i, 1]
            kps[i, lo:hi, 2] = torch.randint(1, 3, (hi - lo, ), generator=g).float()
        out['gt_bboxes'].append(boxes)
        out['gt_labels'].append(labels)
        out['gt_keypoints'].append(kps)
    return out


def _on_canvas(batch, canvas=CANVAS):
    """the batch with plain lists on the device, its image collated to the canvas by torch alone"""
    img = torch.zeros((batch['img'].shape[0], 3) + tuple(canvas), device='cuda')
    img[:, :, :batch['img'].shape[2], :batch['img'].shape[3]] = batch['img'].cuda()
    out = dict(batch, img=img)
    for k in ('gt_bboxes', 'gt_labels', 'gt_keypoints'):
        out[k] = [t.cuda() for t in batch[k]]
    return out


def _grads(model, data):
    model.zero_grad(set_to_none=True)
    out = rn.batch_processor(model, data)
    out['loss'].backward()
    torch.cuda.synchronize()
    return ({n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None},
            {k: v.detach().clone() for k, v in out['log_vars'].items()})


def test_forward_train_on_a_static_batch_equals_the_plain_lists_bit_for_bit():
    from kgdet_amd.static_batch import StaticBatch
    model, _, _ = _make()
    static = StaticBatch.for_model(model, 2, CANVAS, 8, 'cuda')
    # a full-canvas batch first, then the smaller one under test: stale pixels, stale rows and a stale table would all show
    static.load(_batch((8, 5), [(256, 320), (256, 320)], seed=1))
    small = _batch((1, 3), [(192, 256), (224, 288)], seed=2)
    static.load(small)
    plain = _on_canvas(small)
    assert torch.equal(static.img, plain['img'])
    assert static.table.tolist() == [[1, 6, 8, 0], [3, 7, 9, 0]]
    _grads(model, plain)                      # (kernel selection, first packs)
    want, want_losses = _grads(model, plain)
    got, got_losses = _grads(model, static.as_batch())
    assert set(got_losses) == set(want_losses) and len(want) > 100
    for k in want_losses:
        assert torch.equal(got_losses[k], want_losses[k]), (k, got_losses[k], want_losses[k])
    bad = [n for n in want if not torch.equal(got[n], want[n])]
    assert not bad, 'gradients differ between the table route and the plain lists: %s' % bad[:8]
