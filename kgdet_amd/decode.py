"""Final-stage maps -> candidate boxes, scores and landmarks of a whole batch: the one decode of the KGDet head and of the
serial / parallel heads (KP3:825-914, SER:667-750), with no per-image or per-level copy of the arithmetic.

What differs between the two head families is passed in as plain arguments:
* ``clamp_axis``: the KGDet head clamps the landmarks' coordinate axis (x to W, y to H); the serial heads keep the reference's
  slices ``0::3`` / ``1::3`` over the LANDMARK axis (SER:723-724).  Boxes are clamped alike, to ``img_shape`` itself.
* ``true_divide``: the serial heads rescale with a true division by a tensor; the KGDet head divides by a python number, which
  torch computes as ``x * (1 / s)`` on the GPU.
"""
import numpy as np
import torch


def per_image(values, device):
    """python numbers, one per image -> a scalar when they agree, else a [B, 1] tensor uploaded without blocking"""
    if all(v == values[0] for v in values):
        return values[0]
    t = torch.tensor(values, dtype=torch.float32)
    if torch.device(device).type != 'cpu':
        t = t.pin_memory().to(device, non_blocking=True)
    return t.unsqueeze(1)


def class_scores(cls_score, sigmoid=True):
    """class map [B, C, H, W] -> probabilities [B, H*W, C].  An image's scores do not depend on the batch it is decoded in: the
    GPU's kernels round alike at every position; torch's CPU kernels send the last elements of a tensor (what is left after the
    32-wide vector steps) through a scalar routine that rounds up to two ulps differently, so there each image is a tensor of
    its own"""
    B, C = cls_score.shape[:2]
    logits = cls_score.permute(0, 2, 3, 1).reshape(B, -1, C)
    prob = torch.sigmoid if sigmoid else (lambda t: t.softmax(-1))
    return prob(logits) if logits.is_cuda else torch.stack([prob(one) for one in logits])


def top_candidates(scores, nms_pre, sigmoid=True):
    """rows [B, nms_pre] of the locations with the highest per-location maximum (softmax: over the columns after the
    background's), or None where the level has no more than ``nms_pre`` locations and all of them stay"""
    if nms_pre <= 0 or scores.shape[1] <= nms_pre:
        return None
    ranked = scores if sigmoid else scores[..., 1:]
    return ranked.max(dim=2)[0].topk(nms_pre, dim=1)[1]


def gather_rows(t, top):
    """rows ``top`` [B, k] of t [B, n, ...]"""
    index = top.view(top.shape + (1, ) * (t.dim() - 2)).expand(top.shape + t.shape[2:])
    return torch.gather(t, 1, index)


def _clamp(t, lim):
    """to [0, lim]: ``img_shape`` itself, not ``img_shape - 1`` (KP3:882-888); ``lim`` a number or one value per image [B, 1]"""
    if isinstance(lim, (int, float)):
        return t.clamp(min=0, max=lim)
    return torch.minimum(t.clamp(min=0), lim.view((-1, ) + (1, ) * (t.dim() - 1)))


def decode_level(scores, bbox_pred, kpt_pred, points, stride, lim_w, lim_h, nms_pre, num_kpt, clamp_axis, sigmoid=True):
    """One level, all images: boxes [B, n, 4], scores [B, n, C], landmarks [B, n, K, 3] in image coordinates.

    ``scores`` is the level's class map [B, C, H, W], with ``bbox_pred`` [B, 4, H, W] and ``kpt_pred`` [B, K * 2 or 3, H, W]; the
    ``nms_pre`` best locations are kept.  Or it is ``(scores [B, k, C], centres [B, k, 2])`` of candidates chosen beforehand, and
    ``bbox_pred`` / ``kpt_pred`` hold THEIR rows as [B, 4, k, 1] / [B, K ch, k, 1]."""
    selected = isinstance(scores, tuple)
    scores, ctr = scores if selected else (class_scores(scores, sigmoid), None)
    B = scores.shape[0]
    ch = kpt_pred.size(1) // num_kpt
    assert ch == 2 or ch == 3
    bbox_pred = bbox_pred.permute(0, 2, 3, 1).reshape(B, -1, 4)
    kpt_pred = kpt_pred.permute(0, 2, 3, 1).reshape(B, -1, num_kpt, ch)
    if ch == 2:     # visibility not predicted: 1
        kpt_pred = torch.cat([kpt_pred, kpt_pred.new_ones(kpt_pred[..., :1].shape)], dim=-1)
    if not selected:
        ctr = points[:, :2].unsqueeze(0).expand(B, -1, -1)
        top = top_candidates(scores, nms_pre, sigmoid)
        if top is not None:
            ctr, bbox_pred, kpt_pred, scores = (gather_rows(t, top) for t in (ctr, bbox_pred, kpt_pred, scores))
    bboxes = bbox_pred * stride + torch.cat([ctr, ctr], dim=2)
    kpts = kpt_pred.clone()
    kpts[..., :2] = kpts[..., :2] * stride + ctr.unsqueeze(2)
    bboxes = torch.stack([_clamp(bboxes[..., 0], lim_w), _clamp(bboxes[..., 1], lim_h), _clamp(bboxes[..., 2], lim_w),
                          _clamp(bboxes[..., 3], lim_h)], dim=-1)
    if clamp_axis == 'coordinate':
        ix, iy = (Ellipsis, 0), (Ellipsis, 1)
    else:           # 'landmark', the reference quirk: every third landmark's (x, y, v) to W, the next one's to H
        ix, iy = (Ellipsis, slice(0, None, 3), slice(None)), (Ellipsis, slice(1, None, 3), slice(None))
    kpts[ix] = _clamp(kpts[ix], lim_w)
    kpts[iy] = _clamp(kpts[iy], lim_h)
    return bboxes, scores, kpts


def decode_batch(head, cls_scores, bbox_preds, kpt_preds, img_metas, cfg, rescale, clamp_axis, true_divide):
    """Every level decoded and concatenated, then rescaled: boxes [B, M, 4], scores [B, M, C] (no background column) and
    landmarks -- [B, M, 3K] when rescaling, [B, M, K, 3] otherwise, as the reference leaves them (KP3:895-900).
    ``cls_scores[i]`` is a class map or a pre-selected ``(scores, centres)`` pair, see ``decode_level``."""
    first = cls_scores[0][0] if isinstance(cls_scores[0], tuple) else cls_scores[0]
    device, B = first.device, first.shape[0]
    lim_w = per_image([float(m['img_shape'][1]) for m in img_metas], device)
    lim_h = per_image([float(m['img_shape'][0]) for m in img_metas], device)
    nms_pre = cfg.get('nms_pre', -1)
    decoded = []
    for i, (c, b, k) in enumerate(zip(cls_scores, bbox_preds, kpt_preds)):
        points = None if isinstance(c, tuple) else head.point_generators[i].grid_points(c.shape[-2:], head.point_strides[i],
                                                                                      device=device)
        decoded.append(decode_level(c, b, k, points, head.point_strides[i], lim_w, lim_h, nms_pre, head.num_keypts, clamp_axis,
                                    head.use_sigmoid_cls))
    bboxes, scores, kpts = (torch.cat([d[j] for d in decoded], dim=1) for j in range(3))
    if not rescale:
        return bboxes, scores, kpts
    factors = [m['scale_factor'] for m in img_metas]
    if not all(isinstance(f, (int, float)) for f in factors):
        # arrays and numpy scalars: new_tensor() (a blocking upload per image) and a true division, in either head
        sf = torch.stack([bboxes.new_tensor(f) for f in factors])
        bboxes = bboxes / sf.view(B, 1, -1)
        kpts[..., :2] = kpts[..., :2] / sf.view(B, 1, 1, -1)
        return bboxes, scores, kpts.reshape(B, kpts.shape[1], -1)
    sf = per_image([float(f) for f in factors], device)
    if true_divide and isinstance(sf, float):       # a fill kernel, not an upload: capturable in a graph
        sf = torch.full((B, 1), sf, dtype=torch.float32, device=device)
    if torch.is_tensor(sf) and not true_divide and bboxes.is_cuda:
        # torch divides by a python number as x * (1 / s) on the GPU (and truly on the CPU): the same, image by image
        inv = torch.reciprocal(sf)
        bboxes = bboxes * inv.view(B, 1, 1)
        kpts[..., :2] = kpts[..., :2] * inv.view(B, 1, 1, 1)
    else:
        bboxes = bboxes / (sf.view(B, 1, 1) if torch.is_tensor(sf) else sf)
        kpts[..., :2] = kpts[..., :2] / (sf.view(B, 1, 1, 1) if torch.is_tensor(sf) else sf)
    return bboxes, scores, kpts.reshape(B, kpts.shape[1], -1)


def pack_rows(det, label, kp, count):
    """fused-NMS outputs (det [B, M, 5], labels [B, M], landmarks [B, M, 3K], count [B]) -> ONE tensor [B, M, 7 + 3K]: box (4),
    score, label, count (repeated), landmarks"""
    B, M = label.shape
    return torch.cat([det, label.unsqueeze(-1).float(), count.view(B, 1, 1).expand(B, M, 1).float(), kp], dim=-1)


def unpack_results(packed):
    """host copy (numpy) of ``pack_rows``' tensor -> per image (det [n, 5], labels [n] int64, landmarks [n, 3K])"""
    out = []
    for b in range(packed.shape[0]):
        n = int(packed[b, 0, 6])
        out.append((packed[b, :n, :5], packed[b, :n, 5].astype(np.int64), packed[b, :n, 7:]))
    return out
