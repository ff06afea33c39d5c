"""float64 reference of the fused serial / parallel head loss kernels (csrc/serial_loss.hip): the init (PointAssigner) and refine
(MaxIoUAssigner) assignments over a pyramid and the five loss families per level.

Plain numpy, no GPU, no torch.  tests/test_serial_loss_refs.py pins it to the torch chain (heads_serial's loss in float64) and to
the reference project's recorded losses on the CPU; tests/test_gpu_serial_loss_kernels.py holds the kernels to it through the
C ABI.  As in tests/head_loss_refs.py the DISCRETE part and the CONTINUOUS part are kept apart:
  init_distances / init_reference   the PointAssigner metric in float64 on a gt's own level (+inf elsewhere), the level rule,
                                    and the assignment it decides; head_loss_refs.check_assignment says what any correct
                                    assigner satisfies within the rounding of a float32 distance
  refine_reference                  bbox_overlaps + assign_max_iou restated in numpy float32, one rounding per operation in the
                                    order of kgdet_amd.points: the kernel's IoU is bit-equal, so this part is compared exactly
  losses_and_grads                  float64 losses / gradients of GIVEN assignments; ``f32=True``: the kernel's expressions
                                    rounded once per operation with serial sums -- used only to size the bars (bars)
  CASES / make_case / PINNED        the generated and the hand-made inputs of the GPU file
Points of an image are ordered level-major, row-major inside a level (the workspace order of include/kgdet_hip.h).
"""
import numpy as np

from tests import head_loss_refs as H
from tests import step_refs as S

U = S.U
f32, f64 = np.float32, np.float64
M, DECIDED = H.M, H.DECIDED
FAMILIES = ('cls', 'box_init', 'box_refine', 'kpt_init', 'kpt_refine')
NAMES = ('loss_cls', 'loss_bbox_init', 'loss_bbox_refine', 'loss_kpt_init', 'loss_kpt_refine')
STAGE = (1, 0, 1, 0, 1)            # which num_total a family divides by: 0 init, 1 refine
BETA = (None, 0, 1, 2, 3)          # index into cfg beta
# floors of the bars in roundings of the output (head_loss_refs.FLOOR); the keypoint weight 1 / (2 n) has the same count of
# operations as the KGDet head's 4 / (2 n) restated as 1 / (2 n) * 4 minus one product: the floors are kept as they are
FLOOR = {'loss': H.FLOOR['loss'], 'cls': H.FLOOR['cls'], 'box': H.FLOOR['bbox'], 'kpt': H.FLOOR['kpt']}


def kind_of(k):
    return 'cls' if k == 0 else ('box' if k < 3 else 'kpt')


# ---------------------------------------------------------------------------------------------- the case
class Case(object):
    """one call of kgdet_serial_loss_forward / _backward: level shapes, ground truth, configuration, float32 maps
    (maps[family][level] = [B, channels, H, W])"""

    def __init__(self, **kw):
        self.labels = None
        self.__dict__.update(kw)

    @property
    def L(self):
        return len(self.strides)

    @property
    def sizes(self):
        return [h * w for h, w in self.shapes]

    @property
    def N(self):
        return sum(self.sizes)

    @property
    def offsets(self):
        return np.concatenate([[0], np.cumsum(self.sizes)]).astype(int)

    def extents(self, b, l):
        h, w = self.shapes[l]
        return H.extent(self.valid[b][l][0], h), H.extent(self.valid[b][l][1], w)

    def valid_mask(self, b):
        return np.concatenate([H.valid_mask(h, w, *self.valid[b][l]) for l, (h, w) in enumerate(self.shapes)])

    def level_of_points(self):
        return np.concatenate([np.full(n, l) for l, n in enumerate(self.sizes)])

    def centres(self):
        """(px, py, stride) of every point of an image, float32"""
        px, py, st = [], [], []
        for (h, w), s in zip(self.shapes, self.strides):
            x, y = H.grid_points(s, h, w)
            px.append(x)
            py.append(y)
            st.append(np.full(h * w, s, f32))
        return np.concatenate(px), np.concatenate(py), np.concatenate(st)


def pyramid(img_h, img_w, strides=(8, 16, 32, 64, 128)):
    return [(-(-img_h // s), -(-img_w // s)) for s in strides]


# ---------------------------------------------------------------------------------------------- init: PointAssigner
def level_expression(boxes, scale):
    """(log2(w / scale) + log2(h / scale)) / 2 in float64 on the float32 clamped sizes"""
    _, _, w, h = H.centre_size(boxes)
    return (np.log2(w.astype(f64) / scale) + np.log2(h.astype(f64) / scale)) / 2


def gt_levels(case, b):
    """level index of every gt of image b: the expression truncated towards zero, relative to the first stride's log2, clamped"""
    e = level_expression(case.boxes[b], case.scale)
    return np.clip(np.trunc(e).astype(int) - int(np.log2(case.strides[0])), 0, case.L - 1)


def init_distances(case, b):
    """[G, N] float64: the PointAssigner metric of every gt to the valid points of ITS level, +inf elsewhere"""
    lv = gt_levels(case, b)
    D = np.full((len(case.boxes[b]), case.N), np.inf)
    off = case.offsets
    for g, l in enumerate(lv):
        h, w = case.shapes[l]
        D[g, off[l]:off[l + 1]] = H.distances(case.boxes[b][g:g + 1], case.strides[l], h, w, *case.valid[b][l])[0]
    return D


def init_reference(case, b):
    D = init_distances(case, b)
    return H.assign_from_selection(D, H.reference_selection(D, case.pos_num))


def init_margins(case):
    """the smallest cut / contest margin over every (image, gt) and the smallest distance of a level expression from an integer"""
    cuts, contests, lev = [], [], []
    for b in range(case.B):
        c, t = H.assignment_margins(init_distances(case, b), case.pos_num)
        cuts.append(c)
        contests.append(t)
        e = level_expression(case.boxes[b], case.scale)
        lev.append(np.abs(e - np.round(e)))
    return float(np.concatenate(cuts).min()), float(np.concatenate(contests).min()), float(np.concatenate(lev).min())


# ---------------------------------------------------------------------------------------------- refine: MaxIoUAssigner
def image_boxes(case, b):
    """[N, 4] float32: centre + box_init * stride, one rounding per operation (what heads_serial hands its refine assigner)"""
    px, py, st = case.centres()
    raw = np.concatenate([case.maps['box_init'][l][b].reshape(4, -1) for l in range(case.L)], 1)       # [4, N]
    c = np.stack([px, py, px, py])
    return (c + (raw * st[None]).astype(f32)).astype(f32).T


def overlaps_f32(gt, boxes):
    """points.bbox_overlaps(gt, boxes) (mode 'iou', +1 convention) in numpy float32, in its order of operations: [G, N]"""
    g, p = np.asarray(gt, f32)[:, None, :], np.asarray(boxes, f32)[None, :, :]
    one, zero = f32(1), f32(0)
    ew = np.maximum(np.minimum(g[..., 2], p[..., 2]) - np.maximum(g[..., 0], p[..., 0]) + one, zero)
    eh = np.maximum(np.minimum(g[..., 3], p[..., 3]) - np.maximum(g[..., 1], p[..., 1]) + one, zero)
    shared = ew * eh
    area1 = (g[..., 2] - g[..., 0] + one) * (g[..., 3] - g[..., 1] + one)
    area2 = (p[..., 2] - p[..., 0] + one) * (p[..., 3] - p[..., 1] + one)
    out = shared / (area1 + area2 - shared)
    assert out.dtype == f32
    return out


def assign_max_iou(ov, pos_iou_thr, neg_lo, neg_hi, min_pos_iou, valid):
    """points.assign_max_iou (gt_max_assign_all) on a float32 [G, N] overlap matrix, thresholds as float32: ([N] -1 / 0 / gt + 1,
    [N] best overlap, -2 at invalid points)"""
    ov = np.where(valid[None], ov, f32(-2)).astype(f32)
    G = ov.shape[0]
    best, best_gt = ov.max(0), ov.argmax(0)                       # (argmax: the first maximum)
    top = ov.max(1)
    out = np.full(ov.shape[1], -1, np.int64)
    out = np.where((best >= f32(neg_lo)) & (best < f32(neg_hi)), 0, out)
    out = np.where(best >= f32(pos_iou_thr), best_gt + 1, out)
    takes = (ov == top[:, None]) & (top >= f32(min_pos_iou))[:, None]
    last = (takes * np.arange(1, G + 1)[:, None]).max(0)
    out = np.where(last > 0, last, out)
    return np.where(valid, out, 0), best


def refine_reference(case, b):
    return assign_max_iou(overlaps_f32(case.boxes[b], image_boxes(case, b)), case.pos_iou_thr, case.neg_lo, case.neg_hi,
                          case.min_pos_iou, case.valid_mask(b))


# ---------------------------------------------------------------------------------------------- the continuous part
def num_totals(assigned_init, assigned_refine):
    return H.num_total(assigned_init), H.num_total(assigned_refine)


def _rows(case, b, l, k, a):
    """raw prediction [ch, Nl], grid coordinate [ch, Nl], gathered target [ch, Nl], weight mask [ch, Nl] and the per-point
    visible-keypoint count of family k (1..4) on level l of image b under the level's slice ``a`` of the stage's assignment"""
    h, w = case.shapes[l]
    px, py = H.grid_points(case.strides[l], h, w)
    pos, own = a > 0, np.maximum(a - 1, 0)
    raw = case.maps[FAMILIES[k]][l][b].reshape(-1, h * w)
    if k < 3:                      # channels (x1, y1, x2, y2)
        centre = np.stack([px, py, px, py])
        target = np.asarray(case.boxes[b], f32)[own].T
        return raw, centre, target, np.broadcast_to(pos[None], raw.shape), None
    K = case.K                     # channel pairs are (y, x); the targets (x, y)
    centre = np.stack([py, px] * K)
    kp = np.asarray(case.kps[b], f32)
    target = kp[:, :, [1, 0]].reshape(-1, 2 * K)[own].T
    vis = kp[:, :, 2] != 0
    return raw, centre, target, np.repeat(vis, 2, axis=1)[own].T & pos[None], vis.sum(1)[own]


def losses_and_grads(case, assigned_init, assigned_refine, f32=False, grad_of=None, want_losses=True):
    """losses [5, L], (num_total_init, num_total_refine) and the gradient maps ``grad_of`` (a set of (family, level); None: all;
    a dict (k, l) -> [B, ch, Nl]) of ``case`` under the per-image assignments (lists of [N] ints), in float64 -- or, with ``f32``,
    in float32 with one rounding per operation of the kernel's expressions and serial sums.
      decode     centre + raw * stride; keypoint channel pairs (y, x) meet (x, y) targets
      weights    box: 1 on the stage's positives; keypoint: 1 / (2 n_visible) on visible keypoints of positives; label weight
                 pos_weight on refine positives, 1 on valid refine negatives, 0 on don't-care and invalid points
      loss_kl    loss_weight_k * sum_kl / num_total(stage of k);  grad = upstream_kl * loss_weight_k / num_total * d sum_kl"""
    T = np.float32 if f32 else f64
    L = case.L
    totals = num_totals(assigned_init, assigned_refine)
    lw = np.asarray(case.loss_weight, np.float32).astype(T)
    up = np.asarray(case.upstream, np.float32).astype(T).reshape(5, L)
    if grad_of is None:
        grad_of = {(k, l) for k in range(5) for l in range(L)}
    sums = [[T(0)] * L for _ in range(5)]
    grads = {key: [] for key in grad_of}
    off = case.offsets
    for b in range(case.B):
        ai, ar = np.asarray(assigned_init[b], np.int64), np.asarray(assigned_refine[b], np.int64)
        inside = case.valid_mask(b)
        assert not ((ai > 0) & ~inside).any() and not ((ar != 0) & ~inside).any()
        lab = case.labels[b] if case.labels is not None else None
        for l in range(L):
            sl = slice(off[l], off[l + 1])
            stride = T(np.float32(case.strides[l]))
            nt = T(np.float32(np.float32(case.point_base_scale) * np.float32(case.strides[l])))
            for k in range(5):
                if not want_losses and (k, l) not in grads:
                    continue
                gscale = up[k, l] * lw[k] / T(totals[STAGE[k]])
                if k == 0:
                    a = ar[sl]
                    label = np.where(a > 0, 1 if lab is None else np.asarray(lab, np.int64)[np.maximum(a - 1, 0)], 0)
                    label_w = np.where(a > 0, f64(np.float32(case.pos_weight)), ((a == 0) & inside[sl]).astype(f64))
                    x = case.maps['cls'][l][b].reshape(case.C, -1).T                      # [Nl, C]
                    gamma, alpha = np.float32(case.gamma), np.float32(case.alpha)
                    if f32:
                        v = S.focal_forward_f32(x, label, gamma, alpha) * label_w.astype(T)[:, None]
                        sums[0][l] = H._serial_sum(sums[0][l], v)
                        if (0, l) in grads:
                            g = S.focal_backward_f32(x, label, np.ones((1, 1), T), gamma, alpha) * label_w.astype(T)[:, None] * gscale
                            grads[(0, l)].append(g.T)
                    else:
                        sums[0][l] += np.sum(S.focal_forward(x, label, f64(gamma), f64(alpha)) * label_w[:, None])
                        if (0, l) in grads:
                            grads[(0, l)].append(S.focal_backward(x, label, (label_w * gscale)[:, None], f64(gamma), f64(alpha)).T)
                    continue
                a = (ai if STAGE[k] == 0 else ar)[sl]
                beta = np.float32(case.beta[BETA[k]])
                raw, centre, target, mask, nvis = _rows(case, b, l, k, a)
                if k < 3:
                    w = mask.astype(T)
                elif f32:
                    with np.errstate(all='ignore'):
                        kp_w = np.where(nvis > 0, T(1) / (2 * nvis).astype(T), T(0)).astype(T)
                    w = np.where(mask, kp_w[None], T(0)).astype(T)
                else:
                    with np.errstate(all='ignore'):
                        w = np.where(mask, np.where(nvis > 0, 1.0 / (2.0 * nvis), 0.0)[None], 0.0)
                if f32:
                    pred = centre + raw * stride
                    v, g = S.smooth_l1_f32(pred, target, w, gscale, beta, nt)
                    sums[k][l] = H._serial_sum(sums[k][l], v[w != 0])
                    if (k, l) in grads:
                        grads[(k, l)].append(np.where(w != 0, g * stride, T(0)).astype(T))
                else:
                    pred = centre.astype(f64) + raw.astype(f64) * stride
                    sel = w != 0
                    sums[k][l] += S.smooth_l1_sum(pred[sel], target[sel], w[sel], f64(beta), nt)
                    if (k, l) in grads:
                        grads[(k, l)].append(S.smooth_l1_grad(pred, target, w, gscale, f64(beta), nt) * stride)
    losses = np.array([[lw[k] * (sums[k][l] / T(totals[STAGE[k]])) for l in range(L)] for k in range(5)], T)
    return losses, totals, {key: np.stack(v) for key, v in grads.items()}


def bars(ref, res):
    """Bars of the 5 x L losses and of the gradient maps present in both results of losses_and_grads (float64 ``ref``, float32
    ``res`` on the same inputs), by head_loss_refs.bars' rule: 4 x the float32 restatement's own error as a fraction of the
    output's scale -- |loss|, max |gradient| of a map --, pooled over the levels of a family for the losses, but not less than the
    floor.  Returns (loss_bar [5, L], {(k, l): gradient bar})."""
    l64, l32 = ref[0], res[0].astype(f64)
    loss_bar = np.zeros(l64.shape)
    for k in range(5):
        frac = max([abs(l32[k, l] - l64[k, l]) / abs(l64[k, l]) for l in range(l64.shape[1]) if l64[k, l] != 0] + [FLOOR['loss'] * U])
        loss_bar[k] = 4 * frac * np.abs(l64[k])
    grad_bar = {}
    for key in ref[2]:
        if key not in res[2]:
            continue
        scale = float(np.abs(ref[2][key]).max())
        err = float(np.abs(res[2][key].astype(f64) - ref[2][key]).max())
        grad_bar[key] = 4 * max(err, FLOOR[kind_of(key[0])] * U * scale)
    return loss_bar, grad_bar


# ---------------------------------------------------------------------------------------------- generated inputs
DEFAULT_CFG = dict(pos_weight=1.0, gamma=2.0, alpha=0.25, beta=(0.11,) * 4, loss_weight=(1.0, 0.5, 1.0, 2.0, 4.0),
                   pos_iou_thr=0.5, neg_lo=0.0, neg_hi=0.4, min_pos_iou=0.0, scale=4.0, point_base_scale=4.0)
VARIED_CFG = dict(pos_weight=2.5, gamma=0.0, alpha=0.5, beta=(1.0 / 9.0, 2.0, 0.11, 1.0), loss_weight=(1.25, 0.75, 0.0, 1.5, 0.3),
                  pos_iou_thr=0.6, neg_lo=0.1, neg_hi=0.35, min_pos_iou=0.3, scale=4.0, point_base_scale=4.0)


def _spec(**kw):
    d = dict(B=1, img=(64, 96), C=13, K=294, pos_num=1, n_gt=None, pad=None, cfg=DEFAULT_CFG, seed=0, labels='random',
             upstream='ones')
    d.update(kw)
    return d


# name -> spec.  ``seed``: the first of seed, seed + 1000, ... whose init margins all exceed DECIDED and whose level expressions
# all lie DECIDED away from an integer (tests/test_serial_loss_refs.py asserts that the committed seed does).  ``pad``: per image
# the pad_shape (rows, columns) its valid extents follow from (None: the whole image).
CASES = {
    # 64 x 96: levels 8 x 12, 4 x 6, 2 x 3, 1 x 2, 1 x 1 -- a partial second 64-point tile, one-point levels
    'small_b1': _spec(B=1, n_gt=[2], seed=0),
    'small_b2': _spec(B=2, n_gt=[3, 1], seed=1, upstream='varied'),
    'small_b16': _spec(B=16, n_gt=[1, 7, 2, 3] * 4, seed=2),
    'small_null_labels': _spec(B=2, n_gt=[2, 2], labels=None, seed=3),
    # every level of more than one point partly invalid in image 0 (pad 40 x 56 of 64 x 96: 5 x 7, 3 x 4, 2 x 2, 1 x 1, 1 x 1)
    'small_mixed_valid': _spec(B=2, n_gt=[2, 3], pad=[(40, 56), None], seed=4),
    'small_varied_cfg': _spec(B=2, n_gt=[3, 2], cfg=VARIED_CFG, seed=5, upstream='varied'),
    # 256 x 320: 1280 + 320 + 80 + 20 + 6 points, level boundaries off the tile size; 1, 7 and 64 gts in one call
    'mid_mixed_64_1_7': _spec(B=3, img=(256, 320), n_gt=[64, 1, 7], seed=1006),
    # pos_num 3: every level holds at least 3 valid points (the last one 2 x 3)
    'mid_b2_pos3': _spec(B=2, img=(256, 320), n_gt=[3, 2], pos_num=3, pad=[None, (200, 300)], seed=7, upstream='varied'),
    'mid_varied_pos3': _spec(B=2, img=(256, 320), n_gt=[4, 3], pos_num=3, cfg=VARIED_CFG, seed=9, upstream='varied'),
    # group B: the full pyramid 100 x 168 ... 7 x 11 with 8 keypoints: the level sizes, grid limits and stride loops of the real
    # workload without a 100 MB float64 reference
    'full_pyramid_k8': _spec(B=2, img=(800, 1344), K=8, n_gt=[5, 3], seed=8),
}


def _gt_boxes(rng, G, img_h, img_w):
    """sizes log-uniform over the pyramid's range (and beyond both ends), centres inside the image"""
    w = np.exp(rng.uniform(np.log(6.0), np.log(1.2 * max(img_w, 600)), G))
    h = np.exp(rng.uniform(np.log(6.0), np.log(1.2 * max(img_h, 600)), G))
    cx, cy = rng.uniform(0, img_w, G), rng.uniform(0, img_h, G)
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(f32)


def _geometry(sp, seed):
    rng = np.random.default_rng(seed)
    return [_gt_boxes(rng, g, *sp['img']) for g in sp['n_gt']]


def _shell(sp, boxes):
    strides = (8, 16, 32, 64, 128)
    shapes = pyramid(*sp['img'], strides)
    pads = sp['pad'] or [None] * sp['B']
    valid = [[(0, 0) if pads[b] is None else (min(-(-pads[b][0] // s), h), min(-(-pads[b][1] // s), w))
              for s, (h, w) in zip(strides, shapes)] for b in range(sp['B'])]
    up = np.ones(5 * len(strides), f32)
    if sp['upstream'] == 'varied':
        up = np.asarray([1.0, 0.5, -2.0, 0.0, 1.5, 0.7, 1.0, -0.25, 3.0, 0.1] * 3, f32)[:5 * len(strides)]
    return Case(B=sp['B'], C=sp['C'], K=sp['K'], strides=[float(s) for s in strides], shapes=shapes, valid=valid, boxes=boxes,
                pos_num=sp['pos_num'], upstream=up, maps=None, **sp['cfg'])


def find_seed(sp, tries=200):
    """the first of seed, seed + 1000, ... that leaves every margin above DECIDED (how the committed seeds were found)"""
    for t in range(tries):
        case = _shell(sp, _geometry(sp, sp['seed'] + 1000 * t))
        if min(init_margins(case)) > DECIDED:
            return sp['seed'] + 1000 * t
    raise RuntimeError('no decided seed')


def random_maps(case, rng, planted=3):
    """logits ~ 2 randn; keypoint offsets ~ 4 randn; boxes a few strides around their point, and at ``planted`` points per gt
    (on the level the gt's size suggests) the gt itself with a jitter: IoUs above pos_iou_thr exist"""
    B, C, K = case.B, case.C, case.K
    maps = {n: [] for n in FAMILIES}
    for l, (h, w) in enumerate(case.shapes):
        mk = lambda ch, sc: (rng.standard_normal((B, ch, h, w), dtype=f32) * f32(sc)).astype(f32)
        maps['cls'].append(mk(C, 2.0))
        maps['kpt_init'].append(mk(2 * K, 4.0))
        maps['kpt_refine'].append(mk(2 * K, 4.0))
        for n in ('box_init', 'box_refine'):
            half = rng.uniform(0.3, 5.0, (B, 4, h, w)).astype(f32)
            half[:, :2] *= -1
            maps[n].append(half)
    off = case.offsets
    for b in range(B):
        lv = gt_levels(case, b)
        for g, l in enumerate(lv):
            h, w = case.shapes[l]
            s = case.strides[l]
            px, py = H.grid_points(s, h, w)
            for i in rng.choice(h * w, min(planted, h * w), replace=False):
                gt = case.boxes[b][g].astype(f64) + rng.uniform(-0.08, 0.08, 4) * s
                raw = (gt - np.array([px[i], py[i], px[i], py[i]], f64)) / s
                case_map = maps['box_init'][l][b].reshape(4, -1)
                case_map[:, i] = raw.astype(f32)
    return maps


def make_case(name, with_maps=True):
    sp = CASES[name]
    case = _shell(sp, _geometry(sp, sp['seed']))
    case.name = name
    rng = np.random.default_rng(sp['seed'] + 77)
    img_h, img_w = sp['img']
    labels, kps = [], []
    for b in range(case.B):
        G = sp['n_gt'][b]
        labels.append(rng.integers(1, case.C + 1, G).astype(np.int64))
        xy = np.stack([rng.uniform(0, img_w, (G, case.K)), rng.uniform(0, img_h, (G, case.K))], 2)
        v = (rng.random((G, case.K)) < 0.15) * rng.integers(1, 3, (G, case.K)).astype(f64)
        v[-1] = 0                                               # a gt without a visible keypoint
        if G > 1:
            v[0, 0] = 2.0
        kps.append(np.concatenate([xy, v[:, :, None]], 2).astype(f32))
    case.labels = None if sp['labels'] is None else labels
    case.kps = kps
    if with_maps:
        case.maps = random_maps(case, rng)
    return case


# ---------------------------------------------------------------------------------------------- hand-made exact cases
def _pinned_shell(boxes, img=(64, 96), cfg=DEFAULT_CFG, pos_num=1, K=2, C=3, **over):
    """B = 1, every keypoint visible, boxes of area 1 at every point (raw 0) unless planted"""
    sp = _spec(B=1, img=img, C=C, K=K, pos_num=pos_num, n_gt=[len(boxes)], cfg=dict(cfg, **over))
    case = _shell(sp, [np.asarray(boxes, f32)])
    case.labels = [np.arange(len(boxes), dtype=np.int64) % C + 1]
    rng = np.random.default_rng(99)
    G = len(boxes)
    case.kps = [np.concatenate([rng.uniform(0, 64, (G, K, 2)), np.ones((G, K, 1))], 2).astype(f32)]
    case.maps = random_maps(case, rng, planted=0)
    for l in range(case.L):
        case.maps['box_init'][l][:] = 0
    return case


def plant(case, l, row, col, box):
    """make the init box of point (row, col) of level l the integer image box ``box`` (exact: multiples of 1 / stride)"""
    s = case.strides[l]
    c = np.array([col * s, row * s, col * s, row * s])
    raw = (np.asarray(box, f64) - c) / s
    assert ((raw * s + c) == np.asarray(box, f64)).all() and (raw.astype(f32) == raw).all()
    case.maps['box_init'][l][0, :, row, col] = raw.astype(f32)
    return sum(case.sizes[:l]) + row * case.shapes[l][1] + col


def pinned(name):
    """name -> (case, expected): ``expected`` maps 'init' / 'refine' to {point index: value} that must hold besides the
    reference's own answer"""
    far = [5000.0, 5000.0, 5031.0, 5031.0]
    if name == 'levels_exact_and_clamped':
        # w = h = 32: the level expression is exactly 3 = log2(8): the FIRST level; 8 x 8 lies below it, 4096 x 4096 above the last
        boxes = [[16 - 16, 24 - 16, 16 + 16, 24 + 16], [40 - 4, 8 - 4, 40 + 4, 8 + 4], [-2000, -2040, 2096, 2056]]
        case = _pinned_shell(boxes)
        off = case.offsets
        return case, dict(init={3 * 12 + 2: 1, 1 * 12 + 5: 2, off[4]: 3})
    if name == 'equidistant_gts_earlier_wins':
        # centres 3 below and 3 above the point (3, 5) of level 0: the one nearest point of both, at distance 3 / 32
        boxes = [[40 - 16, 27 - 16, 40 + 16, 27 + 16], [40 - 16, 21 - 16, 40 + 16, 21 + 16]]
        case = _pinned_shell(boxes)
        return case, dict(init={3 * 12 + 5: 1}, init_count=1)
    if name == 'equidistant_points_lower_index':
        # the centre halfway between the points (3, 5) and (3, 6); a second gt halfway between (2, 2) and (3, 2)
        boxes = [[44 - 16, 24 - 16, 44 + 16, 24 + 16], [16 - 16, 20 - 16, 16 + 16, 20 + 16]]
        case = _pinned_shell(boxes)
        return case, dict(init={3 * 12 + 5: 1, 2 * 12 + 2: 2}, init_count=2)
    if name == 'identical_gts':
        # gt 0 == gt 1; three planted boxes: the gt itself (IoU 1: the maximum -> the LAST gt), IoU 0.5 and 0.75 (-> the first)
        boxes = [[10, 10, 29, 29], [10, 10, 29, 29]]
        case = _pinned_shell(boxes)
        top = plant(case, 0, 2, 2, [10, 10, 29, 29])
        half = plant(case, 0, 2, 3, [10, 10, 29, 19])
        three = plant(case, 0, 3, 2, [10, 10, 24, 29])
        return case, dict(refine={top: 2, half: 1, three: 1}, best={top: 1.0, half: 0.5, three: 0.75})
    if name == 'disjoint_gt_claims_all':
        # the second gt overlaps no box: its maximum is exactly 0 >= min_pos_iou = 0 and it takes every valid point at IoU 0 --
        # all of them, as the last gt
        case = _pinned_shell([[10, 10, 29, 29], far])
        p = plant(case, 0, 2, 2, [10, 10, 29, 29])
        return case, dict(refine={p: 2}, refine_all=2)
    if name == 'iou_exactly_at_thresholds':
        # gt 10 x 10 = 100; boxes inside it of area 40 and 50: IoU float32(0.4) is not < neg_hi (don't care), 0.5 is positive;
        # min_pos_iou above 1 keeps the gt-max step out
        case = _pinned_shell([[0, 0, 9, 9]], min_pos_iou=1.5)
        p40 = plant(case, 0, 0, 0, [0, 0, 9, 3])
        p50 = plant(case, 0, 0, 1, [0, 0, 9, 4])
        p30 = plant(case, 0, 1, 0, [0, 0, 9, 2])
        return case, dict(refine={p40: -1, p50: 1, p30: 0}, best={p40: float(f32(0.4)), p50: 0.5, p30: float(f32(0.3))})
    if name == 'tuple_neg_iou_thr':
        # negatives only inside [0.1, 0.4): an IoU of 0 (every unplanted point) is don't-care
        case = _pinned_shell([[0, 0, 9, 9]], neg_lo=0.1, neg_hi=0.4, min_pos_iou=1.5)
        p30 = plant(case, 0, 0, 0, [0, 0, 9, 2])
        p10 = plant(case, 0, 0, 1, [0, 0, 9, 0])
        p05 = plant(case, 0, 1, 0, [0, 0, 4, 0])
        return case, dict(refine={p30: 0, p10: 0, p05: -1, 5: -1}, best={p10: float(f32(0.1))})
    if name == 'no_refine_positive':
        # no IoU reaches pos_iou_thr and min_pos_iou is out of reach: zero refine positives, num_total_refine = max(0, 1)
        case = _pinned_shell([[0, 0, 9, 9], [40, 20, 70, 50]], min_pos_iou=1.5)
        plant(case, 0, 0, 0, [0, 0, 9, 2])
        return case, dict(refine_positives=0)
    raise KeyError(name)


PINNED = ('levels_exact_and_clamped', 'equidistant_gts_earlier_wins', 'equidistant_points_lower_index', 'identical_gts',
          'disjoint_gt_claims_all', 'iou_exactly_at_thresholds', 'tuple_neg_iou_thr', 'no_refine_positive')
