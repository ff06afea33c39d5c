"""float64 reference of the fused head-loss kernels (csrc/head_loss.hip): target assignment + the nine losses of the KGDet head.

Plain numpy, no GPU, no torch.  tests/test_head_loss_refs.py pins it to the torch chain (points.assign_points, point_target_kp_dense,
the head's loss) on the CPU; tests/test_gpu_head_loss_kernels.py holds the kernels to it through the C ABI.

The DISCRETE part (which points a ground truth selects, which ground truth a point goes to) and the CONTINUOUS part (losses and
gradients for a given assignment) are kept apart: a float64 reference cannot arbitrate a float32 near-tie, so the assignment is
never compared as one fixed answer unless the margins say the case is decided.
  distances            the PointAssigner metric in float64
  assignment_margins   how far every (image, gt) is from a tie
  check_assignment     what ANY correct assigner satisfies, within the rounding of a float32 distance (M)
  losses_and_grads     float64 losses / gradients of a GIVEN assignment; ``f32=True``: the same expressions rounded once per
                       operation in float32 with serial sums -- used only to size the bars (bars)
  CASES / make_case    the generated inputs of the GPU file, by regime:
      'decided'   random; the committed seed makes every margin exceed 64 M, so the reference alone decides the assignment
      'exact'     power-of-two sizes, centres on grid points or mid-cells: every float32 operation of the distance is exact,
                  fused or not, so ties are exact ties and the documented rule -- lowest point index, then earliest gt -- holds
      'free'      near-ties on purpose (a non-dyadic square gt; degenerate boxes): only check_assignment's conditions hold
"""
import numpy as np

from tests import step_refs as S

U = S.U
f32, f64 = np.float32, np.float64
MAX_IMAGES, MAX_GT, MAX_POINTS = 16, 64, 4096

# Relative error of a float32 distance sqrt(((px - cx) / w)^2 + ((py - cy) / h)^2) against the float64 value of the same
# expression on the same float32 centre and size: two subtractions, two divisions, two squares, an addition and a square root, one
# rounding of 2^-24 each (a fused multiply-add only removes roundings).  Propagated exactly the bound is 4 U (the squares double
# the error of a quotient, the root halves the sum's); the plain count of 8 is kept: two float32 distances whose float64 values
# are closer than a factor 1 + M may compare either way.
M_ROUNDINGS = 8
M = M_ROUNDINGS * U
DECIDED = 64 * M          # the margin the 'decided' regimes are generated to


# ---------------------------------------------------------------------------------------------- the discrete part
def extent(v, full):
    """valid rows / columns of the ABI: 0 = the whole grid, values beyond it are clamped"""
    return min(int(v), full) if v > 0 else full


def grid_points(stride, H, W):
    """(px, py) of the H * W points, row-major, as the float32 values column * stride and row * stride"""
    px = np.tile(np.arange(W, dtype=f32) * f32(stride), H)
    py = np.repeat(np.arange(H, dtype=f32) * f32(stride), W)
    return px, py


def centre_size(boxes):
    """centre and clamped size of float32 boxes in float32: ONE correctly rounded addition / subtraction each (the halving is
    exact), which every IEEE float32 implementation -- the torch chain, the kernel -- forms identically.  The metric is defined
    on these values."""
    b = np.asarray(boxes, f32).reshape(-1, 4)
    cx, cy = (b[:, 0] + b[:, 2]) / f32(2), (b[:, 1] + b[:, 3]) / f32(2)
    w, h = np.maximum(b[:, 2] - b[:, 0], f32(1e-6)), np.maximum(b[:, 3] - b[:, 1], f32(1e-6))
    return cx, cy, w, h


def valid_mask(H, W, vh, vw):
    vh, vw = extent(vh, H), extent(vw, W)
    return ((np.arange(H) < vh)[:, None] & (np.arange(W) < vw)[None, :]).reshape(-1)


def distances(boxes, stride, H, W, vh=0, vw=0):
    """[G, H * W] float64: |(p - centre) / max(size, 1e-6)| of every point to every gt; +inf at points outside the valid extent"""
    px, py = grid_points(stride, H, W)
    cx, cy, w, h = (a.astype(f64)[:, None] for a in centre_size(boxes))
    dx, dy = (px.astype(f64)[None] - cx) / w, (py.astype(f64)[None] - cy) / h
    d = np.sqrt(dx * dx + dy * dy)
    return np.where(valid_mask(H, W, vh, vw)[None], d, np.inf)


def reference_selection(D, pos_num):
    """[G, N] bool: the pos_num nearest points of every gt under the (distance, point index) order"""
    sel = np.zeros(D.shape, bool)
    for g in range(D.shape[0]):
        sel[g, np.argsort(D[g], kind='stable')[:pos_num]] = True
    return sel


def assign_from_selection(vals, sel):
    """[N] int: per point the selecting gt with the smallest value (+ 1), the earliest on equal values; 0 = none.  ``vals`` are
    the distances the comparison runs on (float64 for the reference, the kernel's float32 for the kernel's own rule)."""
    v = np.where(sel, vals, np.inf)
    owner = np.argmin(v, axis=0)                       # first minimum
    return np.where(sel.any(0), owner + 1, 0).astype(np.int64)


def _rel_gap(a, b):
    """b / a - 1 for 0 <= a <= b: +inf when there is no b, 0 for an exact tie"""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    with np.errstate(all='ignore'):
        return np.where(np.isinf(b), np.inf, np.where(b == a, 0.0, np.where(a > 0, (b - a) / a, np.inf)))


def assignment_margins(D, pos_num):
    """Two relative float64 gaps per gt, (cut [G], contest [G]): between its pos_num-th and (pos_num + 1)-th nearest distance
    (+inf when every valid point is selected), and -- over the points it selects that another gt selects too -- between the
    two smallest of the competing distances (+inf without such a point).  A gap of 0 is an exact tie."""
    s = np.sort(D, axis=1)
    nxt = s[:, pos_num] if pos_num < D.shape[1] else np.full(D.shape[0], np.inf)
    cut = _rel_gap(s[:, pos_num - 1], nxt)
    sel = reference_selection(D, pos_num)
    v = np.sort(np.where(sel, D, np.inf), axis=0)
    gap = _rel_gap(v[0], v[1]) if D.shape[0] > 1 else np.full(D.shape[1], np.inf)
    contest = np.array([np.min(gap[sel[g]], initial=np.inf) for g in range(D.shape[0])])
    return cut, contest


def check_assignment(x, D, pos_num, m=M):
    """What any correct assigner satisfies, for one image.  ``x`` is either the per-gt selections [G, N] (the distance where gt g
    selects point i, +inf elsewhere: the kernel's dsel rows) or a final assignment [N] (0 = none, g + 1).  With selections:
      * every gt selects exactly pos_num points, all of them valid, at a value within m of the float64 distance;
      * no selected point is farther in float64 than (1 + m) x the pos_num-th smallest distance, no unselected one nearer than
        that distance / (1 + m);
      * the assignment follows from the selections by the documented rule (smallest value, the earliest gt on equal values), and
        a point goes to the nearest selecting gt within m; where float64 distances are equal, to the earliest.
    With an assignment alone, the consequences of the same: points of gt g are valid and within (1 + m) x its cut, at most
    pos_num of them; a point some gt selects beyond doubt is assigned, to a gt within m of the nearest such.
    Raises AssertionError; returns the [N] assignment."""
    x = np.asarray(x)
    G, N = D.shape
    kth = np.sort(D, axis=1)[:, pos_num - 1]
    assert np.isfinite(kth).all(), 'fewer valid points than pos_num'
    if x.ndim == 2:
        assert x.shape == (G, N)
        assert not np.isnan(x).any(), 'unwritten selection rows'
        sel = x < np.inf
        for g in range(G):
            n = int(sel[g].sum())
            assert n == pos_num, 'gt %d selects %d points, not %d' % (g, n, pos_num)
            assert np.isfinite(D[g][sel[g]]).all(), 'gt %d selects an invalid point' % g
            far = D[g][sel[g]].max()
            assert far <= kth[g] * (1 + m), 'gt %d selects a point at %.9g, its cut is %.9g' % (g, far, kth[g])
            if n < N:
                near = D[g][~sel[g]].min()
                assert near >= kth[g] / (1 + m), 'gt %d leaves out a point at %.9g, its cut is %.9g' % (g, near, kth[g])
            err = np.abs(x[g][sel[g]].astype(f64) - D[g][sel[g]])
            assert (err <= m * D[g][sel[g]]).all(), 'gt %d: a selected distance is off by more than m' % g
        assigned = assign_from_selection(x, sel)
        assert (assigned[~sel.any(0)] == 0).all()
    else:
        assigned = x.astype(np.int64)
        assert assigned.shape == (N,) and assigned.min() >= 0 and assigned.max() <= G
        srt = np.sort(D, axis=1)
        nxt = srt[:, pos_num] if pos_num < N else np.full(G, np.inf)
        sel = D * (1 + m) < nxt[:, None]                    # selected beyond doubt: nearer than the (pos_num + 1)-th by more than m
        for g in range(G):
            mine = assigned == g + 1
            assert mine.sum() <= pos_num, 'gt %d holds %d points' % (g, mine.sum())
            assert np.isfinite(D[g][mine]).all(), 'gt %d holds an invalid point' % g
            assert (D[g][mine] <= kth[g] * (1 + m)).all(), 'gt %d holds a point beyond its cut' % g
        assert (assigned[sel.any(0)] > 0).all(), 'a point that a gt selects is left unassigned'
    pts = np.flatnonzero(assigned > 0)
    own = assigned[pts] - 1
    sel = sel.copy()
    sel[own, pts] = True                                   # (with an assignment alone: its owner selects the point)
    d_own = D[own, pts]
    assert np.isfinite(d_own).all(), 'an invalid point is assigned'
    best = np.where(sel, D, np.inf)[:, pts].min(0)
    assert (d_own <= best * (1 + m)).all(), 'a point goes to a gt that is not the nearest within m'
    first = np.argmax(np.where(sel, D, np.inf)[:, pts] == d_own[None], axis=0)     # the earliest gt at exactly that distance
    assert (first >= own).all(), 'a later gt keeps an exact tie'
    return assigned


# ---------------------------------------------------------------------------------------------- the continuous part
class Case(object):
    """one call of kgdet_head_loss_forward / _backward: shapes, ground truth, configuration, maps (float32 numpy)"""

    def __init__(self, **kw):
        self.labels = None
        self.__dict__.update(kw)

    @property
    def N(self):
        return self.H * self.W

    def extents(self, b):
        return extent(self.valid[b][0], self.H), extent(self.valid[b][1], self.W)

    def distances(self, b):
        return distances(self.boxes[b], self.stride, self.H, self.W, *self.valid[b])


def num_total(assigned):
    """sum over the images of max(positives, 1)"""
    return int(sum(max(int((a > 0).sum()), 1) for a in assigned))


def _serial_sum(acc, terms):
    """acc + t0 + t1 + ... one float32 addition at a time (numpy's cumsum is that loop)"""
    if terms.size == 0:
        return acc
    return np.cumsum(np.concatenate([np.array([acc], f32), terms.astype(f32).reshape(-1)]), dtype=f32)[-1]


def _point_context(case, b, a):
    """per point of image b under assignment a: positive mask, own gt, focal label, label weight (float64 values)"""
    pos = a > 0
    own = np.maximum(a - 1, 0)
    lab = case.labels[b] if case.labels is not None else None
    label = np.where(pos, 1 if lab is None else np.asarray(lab, np.int64)[own], 0)
    vh, vw = case.extents(b)
    inside = valid_mask(case.H, case.W, vh, vw)
    assert not (pos & ~inside).any()
    label_w = np.where(pos, f64(f32(case.pos_weight)), inside.astype(f64))
    return pos, own, label, label_w


def _regression_rows(case, b, kind, stage, pos, own):
    """raw prediction [ch, N], grid coordinate added on decode [ch, N], gathered target [ch, N], visibility-or-positive mask
    [ch, N] and the per-point visible-keypoint count [N] of the box (kind 1) or keypoint (kind 2) rows of one image"""
    px, py = grid_points(case.stride, case.H, case.W)
    if kind == 1:                  # channels (x1, y1, x2, y2): offset_to_pts(y_first=False)
        raw = case.maps['bbox'][stage][b].reshape(4, -1)
        centre = np.stack([px, py, px, py])
        target = np.asarray(case.boxes[b], f32)[own].T
        mask = np.broadcast_to(pos[None], raw.shape)
        return raw, centre, target, mask, None
    K = case.K                     # channel pairs are (y, x); the targets (x, y): channel 2 m takes y of keypoint m
    raw = case.maps['kpt'][stage][b].reshape(2 * K, -1)
    centre = np.stack([py, px] * K)
    kp = np.asarray(case.kps[b], f32)
    target = kp[:, :, [1, 0]].reshape(-1, 2 * K)[own].T
    vis = kp[:, :, 2] != 0
    mask = np.repeat(vis, 2, axis=1)[own].T & pos[None]
    return raw, centre, target, mask, vis.sum(1)[own]


def losses_and_grads(case, assigned, f32=False, grad_of=range(9), want_losses=True):
    """The nine losses, num_total and the gradient maps ``grad_of`` (indices cls 0-2, bbox 3-5, kpt 6-8; a dict k -> [B, ch, N])
    of ``case`` under the per-image assignment ``assigned`` (list of [N] ints), in float64 -- or, with ``f32``, in float32 with one
    rounding per operation of the kernel's expressions and serial sums.
      decode     pred * stride + centre; keypoint channel pairs (y, x) meet (x, y) targets
      targets    box / keypoint of the assigned gt; keypoint weight 4 / (2 n_visible) on visible keypoints, 0 for a gt without one
      label weight   pos_weight on positives, 1 on valid negatives, 0 outside the valid extent
      loss_k     loss_weight_k * sum_k / num_total;  grad = upstream_k * loss_weight_k / num_total * d sum_k
    ``want_losses=False`` evaluates only the rows of ``grad_of`` (the losses returned are then not meaningful)."""
    T = np.float32 if f32 else f64
    total = num_total(assigned)
    nt, stride = T(np.float32(case.normalize_term)), T(np.float32(case.stride))
    lw, up = np.asarray(case.loss_weight, np.float32).astype(T), np.asarray(case.upstream, np.float32).astype(T)
    sums = [T(0)] * 9
    grads = {k: [] for k in grad_of}
    gscale = [up[k] * lw[k] / T(total) for k in range(9)]
    for b in range(case.B):
        a = np.asarray(assigned[b], np.int64)
        pos, own, label, label_w = _point_context(case, b, a)
        for k in range(9):
            kind, stage = divmod(k, 3)
            if not want_losses and k not in grads:
                continue
            if kind == 0:
                x = case.maps['cls'][stage][b].reshape(case.C, -1).T                      # [N, C]
                gamma, alpha = np.float32(case.gamma[stage]), np.float32(case.alpha[stage])
                if f32:
                    l = S.focal_forward_f32(x, label, gamma, alpha) * label_w.astype(T)[:, None]
                    sums[k] = _serial_sum(sums[k], l)
                    if k in grads:
                        g = S.focal_backward_f32(x, label, np.ones((1, 1), T), gamma, alpha) * label_w.astype(T)[:, None] * gscale[k]
                        grads[k].append(g.T)
                else:
                    sums[k] += np.sum(S.focal_forward(x, label, f64(gamma), f64(alpha)) * label_w[:, None])
                    if k in grads:
                        grads[k].append(S.focal_backward(x, label, (label_w * gscale[k])[:, None], f64(gamma), f64(alpha)).T)
                continue
            beta = np.float32(case.beta[k - 3])
            raw, centre, target, mask, nvis = _regression_rows(case, b, kind, stage, pos, own)
            if kind == 1:
                w = mask.astype(T)
            elif f32:
                with np.errstate(all='ignore'):
                    kp_w = np.where(nvis > 0, T(1) / (2 * nvis).astype(T) * T(4), T(0)).astype(T)
                w = np.where(mask, kp_w[None], T(0)).astype(T)
            else:
                with np.errstate(all='ignore'):
                    w = np.where(mask, np.where(nvis > 0, 4.0 / (2.0 * nvis), 0.0)[None], 0.0)
            if f32:
                pred = raw * stride + centre
                l, g = S.smooth_l1_f32(pred, target, w, gscale[k], beta, nt)
                sums[k] = _serial_sum(sums[k], l[w != 0])
                if k in grads:
                    grads[k].append(np.where(w != 0, g * stride, T(0)).astype(T))
            else:
                pred = raw.astype(f64) * stride + centre.astype(f64)
                sel = w != 0
                sums[k] += S.smooth_l1_sum(pred[sel], target[sel], w[sel], f64(beta), nt)
                if k in grads:
                    grads[k].append(S.smooth_l1_grad(pred, target, w, gscale[k], f64(beta), nt) * stride)
    losses = np.array([lw[k] * (sums[k] / T(total)) for k in range(9)], T)
    return losses, total, {k: np.stack(v) for k, v in grads.items()}


# Floors of the bars, in roundings of the output itself (what remains where the float32 restatement happens to be exact):
#   a loss         the last addition of its sum, the division by num_total, the product with loss_weight
#   a cls gradient focal'(x) * label_w * g: the last product of focal', two more products, g = upstream * loss_weight / num_total
#   a bbox / kpt gradient   g * w * dl / nt * stride: four operations and the two of g
FLOOR = {'loss': 3, 'cls': 5, 'bbox': 6, 'kpt': 6}
KINDS = ('cls', 'bbox', 'kpt')


def bars(ref, res):
    """Bars of the nine losses and of the gradient maps present in both results of losses_and_grads (float64 ``ref``, float32
    ``res`` on the same inputs): 4 x the float32 restatement's own error, taken as a fraction of the output's scale -- |loss|
    (its terms are all >= 0), max |gradient| of a map -- and pooled over the three stages of a kind for the losses (one serial
    sum is one draw), but not less than the floor above.  The factor 4 covers what the kernel legitimately does differently:
    butterfly and per-workgroup partial sums instead of a serial one, device expf / logf / powf, fused multiply-adds.
    Returns (loss_bar [9], {k: gradient bar})."""
    l64, l32 = ref[0], res[0].astype(f64)
    loss_bar = np.zeros(9)
    for kind in range(3):
        ks = [3 * kind + s for s in range(3)]
        frac = max([abs(l32[k] - l64[k]) / abs(l64[k]) for k in ks if l64[k] != 0] + [FLOOR['loss'] * U])
        for k in ks:
            loss_bar[k] = 4 * frac * abs(l64[k])
    grad_bar = {}
    for k in ref[2]:
        if k not in res[2]:
            continue
        scale = float(np.abs(ref[2][k]).max())
        err = float(np.abs(res[2][k].astype(f64) - ref[2][k]).max())
        grad_bar[k] = 4 * max(err, FLOOR[KINDS[k // 3]] * U * scale)
    return loss_bar, grad_bar


# ---------------------------------------------------------------------------------------------- generated inputs
DEFAULT_CFG = dict(pos_weight=1.0, gamma=(2.0, 2.0, 2.0), alpha=(0.25, 0.25, 0.25), beta=(1.0 / 9.0,) * 6,
                   loss_weight=(0.5, 0.5, 1.0, 0.5, 0.5, 1.0, 0.5, 0.5, 1.0), upstream=(1.0,) * 9)
VARIED_CFG = dict(pos_weight=2.5, gamma=(0.0, 1.5, 2.0), alpha=(0.25, 0.5, 0.5), beta=(1.0 / 9.0, 0.11, 2.0, 0.11, 2.0, 1.0 / 9.0),
                  loss_weight=(0.5, 0.0, 1.25, 0.75, 2.0, 0.0, 0.0, 1.5, 0.3), upstream=(1.0, 0.5, -2.0, 0.0, 1.5, 0.7, 1.0, -0.25, 3.0))


def _spec(**kw):
    d = dict(B=1, H=25, W=42, C=13, K=294, stride=32.0, pos_num=25, n_gt=None, valid=None, cfg=DEFAULT_CFG, seed=0,
             regime='decided', geometry='random', vis='sparse', labels='random', values='normal', base_scale=4)
    d.update(kw)
    return d


# name -> spec.  ``seed`` of a 'decided' case: the first of seed, seed + 1000, ... whose margins all exceed DECIDED
# (tests/test_head_loss_refs.py asserts that the committed seed does).
CASES = {
    # the training shape; two images of 3 and 5 gts: gmax < 64 with the selection rows 64 apart; 1050 = 16 * 64 + 26 (tail tile)
    'kgdet': _spec(B=2, n_gt=[3, 5]),
    'kgdet_config': _spec(B=2, n_gt=[4, 2], cfg=VARIED_CFG, vis='values_1_2', labels='with_C', valid=[(20, 30), (0, 0)], seed=1),
    # N < 64: one tile with 29 dead lanes; (C, K) = (1, 1): 21 rows in all; labels NULL
    'n35_c1k1': _spec(H=5, W=7, C=1, K=1, pos_num=9, n_gt=[1], labels=None, vis='all', seed=2),
    'n35_b16': _spec(B=16, H=5, W=7, C=1, K=1, pos_num=10, n_gt=[1, 2, 3, 1] * 4, vis='all', seed=3),
    # strips: side = ceil(sqrt(pos_num)) exceeds the one row / column -- every valid point is a candidate (T = FLT_MAX)
    'strip_1xW': _spec(B=2, H=1, W=50, C=1, K=1, pos_num=10, n_gt=[2, 1], seed=4, vis='all'),
    'strip_Hx1': _spec(B=1, H=40, W=1, C=80, K=17, pos_num=1, n_gt=[3], seed=5),
    # 64 gts next to 1 next to 7: blocks of images 1 and 2 return early and leave selection rows unwritten
    'mixed_64_1_7': _spec(B=3, C=80, K=17, pos_num=9, n_gt=[64, 1, 7], geometry='overlapping', seed=6),
    # centres outside the grid on every side and beyond the valid extent, next to the valid border; extents beyond H, W (clamped)
    'outside': _spec(B=4, C=1, K=1, pos_num=25, n_gt=[4, 4, 2, 2], geometry='outside', valid=[(0, 0), (18, 30), (99, 99), (25, 7)],
                     seed=7, vis='all'),
    'border_pos10': _spec(B=2, C=1, K=1, pos_num=10, n_gt=[3, 3], geometry='border', valid=[(11, 17), (0, 0)], seed=8, vis='all'),
    # side > vh or vw: a single valid row, a single valid column; pos_num == vh * vw exactly; pos_num == N
    'one_row_valid': _spec(B=2, C=1, K=1, pos_num=9, n_gt=[2, 2], valid=[(1, 0), (0, 1)], seed=9, vis='all'),
    'pos_num_all_valid': _spec(B=2, H=5, W=7, C=1, K=1, pos_num=12, n_gt=[2, 1], valid=[(3, 4), (4, 3)], seed=10, vis='all'),
    'pos_num_N': _spec(B=1, H=5, W=7, C=13, K=1, pos_num=35, n_gt=[2], seed=11),
    'tiny_and_huge_gts': _spec(B=2, C=1, K=17, pos_num=9, n_gt=[3, 3], geometry='tiny_huge', seed=12, vis='none_and_all'),
    # values
    'saturated_logits': _spec(B=1, H=5, W=7, C=13, K=17, pos_num=9, n_gt=[2], values='saturated', seed=13),
    'scale_1e3': _spec(B=1, H=9, W=11, C=1, K=17, pos_num=9, n_gt=[2], values='1e3', seed=14),
    'scale_1e-3_kink': _spec(B=1, H=9, W=11, C=1, K=17, pos_num=9, n_gt=[2], values='kink', cfg=VARIED_CFG, seed=15),
    'no_visible_keypoint': _spec(B=1, H=9, W=11, C=1, K=17, pos_num=9, n_gt=[2], vis='none', seed=16),
    # the envelope: B = 16, 4096 points (the LDS maximum), 294 keypoints; ~145 MB of maps per side -- the only such case
    'envelope': _spec(B=16, H=64, W=64, pos_num=25, n_gt=[64, 1, 7, 2] * 4, seed=1017, valid=[(0, 0), (64, 40), (33, 64), (70, 70)] * 4),
    # exact ties
    'exact_ties': _spec(B=2, C=13, K=17, pos_num=10, n_gt=[4, 2], regime='exact', geometry='exact'),
    'exact_midcell_pos1': _spec(B=1, H=9, W=11, C=1, K=1, pos_num=1, n_gt=[2], regime='exact', geometry='exact_midcell', vis='all'),
    'identical_64': _spec(B=1, C=1, K=1, pos_num=9, n_gt=[64], regime='exact', geometry='identical', vis='all'),
    # near-ties on purpose
    'inexact_tie': _spec(B=1, C=1, K=1, pos_num=16, n_gt=[1], regime='free', geometry='inexact', vis='all'),
    'degenerate': _spec(B=1, C=1, K=17, pos_num=9, n_gt=[4], regime='free', geometry='degenerate'),
}


def _boxes(sp, rng, b, G, vh, vw):
    s, geo = sp['stride'], sp['geometry']
    ew, eh = vw * s, vh * s                                       # the valid extent in image coordinates
    if geo in ('random', 'overlapping', 'border', 'outside', 'tiny_huge'):
        cx, cy = rng.uniform(0, ew, G), rng.uniform(0, eh, G)
        w, h = rng.uniform(1.5 * s, max(0.6 * ew, 3 * s), G), rng.uniform(1.5 * s, max(0.6 * eh, 3 * s), G)
        if geo == 'overlapping':                                  # all centres within two cells of one another
            cx, cy = ew / 2 + rng.uniform(-2 * s, 2 * s, G), eh / 2 + rng.uniform(-2 * s, 2 * s, G)
        elif geo == 'border':                                     # within a cell of the valid border, inside and outside
            cx[0], cy[0] = ew - s * rng.uniform(0.1, 0.9), eh - s * rng.uniform(0.1, 0.9)
            cx[1], cy[1] = ew + s * rng.uniform(0.1, 0.9), rng.uniform(0, eh)
            cx[2], cy[2] = rng.uniform(0, s), eh - s * rng.uniform(1.0, 1.4)
        elif geo == 'outside':                                    # left / above / right / below the grid or the valid extent
            far = rng.uniform(1.5 * s, 6 * s, 4)
            cx[0] = -far[0]
            cy[1] = -far[1]
            if G > 2:
                cx[2] = sp['W'] * s + far[2]
                cy[3] = sp['H'] * s + far[3]
            else:
                cx[0], cy[1] = ew + far[2], eh + far[3]
        elif geo == 'tiny_huge':
            w[0], h[0] = rng.uniform(0.01, 0.05, 2)
            w[1], h[1] = 3 * sp['W'] * s + rng.uniform(0, s), 2 * sp['H'] * s + rng.uniform(0, s)
        return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(f32)
    if geo == 'exact':
        # power-of-two sizes, centres on grid points: every distance operation is exact.  Image 0: a square gt at (16, 10)
        # whose 10th nearest is one of four points at distance 2 cells (the lowest index wins); a larger one on the same centre;
        # a copy of the first (the earlier keeps everything); one in the corner, clamped block.  Image 1: a rectangle, a copy.
        def box(c, r, w, h):
            return [c * s - w / 2, r * s - h / 2, c * s + w / 2, r * s + h / 2]
        if b == 0:
            return np.array([box(16, 10, 256, 256), box(16, 10, 512, 512), box(16, 10, 256, 256), box(0, 0, 128, 128)][:G], f32)
        return np.array([box(30, 20, 512, 256), box(30, 20, 512, 256)][:G], f32)
    if geo == 'exact_midcell':                                    # equidistant from four grid points: pos_num 1 takes the lowest
        c, r = 4.5, 3.5
        return np.array([[c * s - 64, r * s - 64, c * s + 64, r * s + 64], [c * s - 128, r * s - 64, c * s + 128, r * s + 64]][:G], f32)
    if geo == 'identical':
        return np.tile(np.array([[20 * s - 128, 12 * s - 128, 20 * s + 128, 12 * s + 128]], f32), (G, 1))
    if geo == 'inexact':
        # a square gt of non-dyadic size centred on a grid point: the points (2, 1) and (1, 2) cells away are equidistant in
        # exact arithmetic, and pos_num = 16 cuts through that shell of eight (ranks 13 .. 20)
        half = 150.15
        return np.array([[16 * s - half, 10 * s - half, 16 * s + half, 10 * s + half]], f32)
    if geo == 'degenerate':                                       # w = 0, h = 0, both, and a negative width: all clamp to 1e-6
        c, r = 13 * s + 5.0, 9 * s + 7.0
        return np.array([[c, r - 100, c, r + 100], [c - 90, r, c + 90, r], [c, r, c, r], [c + 10, r - 50, c - 10, r + 50]][:G], f32)
    raise ValueError(geo)


def _geometry(sp, seed):
    rng = np.random.default_rng(seed)
    B, H, W = sp['B'], sp['H'], sp['W']
    valid = sp['valid'] or [(0, 0)] * B
    boxes = []
    for b in range(B):
        boxes.append(_boxes(sp, rng, b, sp['n_gt'][b], extent(valid[b][0], H), extent(valid[b][1], W)))
    return boxes, valid


def margins_of(sp, boxes, valid):
    """the smallest cut and contest margin over every (image, gt), and the share of (image, gt) pairs below M"""
    cuts, contests = [], []
    for b in range(sp['B']):
        D = distances(boxes[b], sp['stride'], sp['H'], sp['W'], *valid[b])
        c, t = assignment_margins(D, sp['pos_num'])
        cuts.append(c)
        contests.append(t)
    cuts, contests = np.concatenate(cuts), np.concatenate(contests)
    undecided = float(np.mean((cuts <= M) | (contests <= M)))
    return float(cuts.min()), float(contests.min()), undecided


def find_seed(sp, tries=200):
    """the first of seed, seed + 1000, ... that leaves every margin above DECIDED (how the committed seeds were found)"""
    for t in range(tries):
        boxes, valid = _geometry(sp, sp['seed'] + 1000 * t)
        cut, contest, _ = margins_of(sp, boxes, valid)
        if min(cut, contest) > DECIDED:
            return sp['seed'] + 1000 * t
    raise RuntimeError('no decided seed')


def make_case(name, with_maps=True):
    sp = CASES[name]
    B, H, W, C, K, s = sp['B'], sp['H'], sp['W'], sp['C'], sp['K'], sp['stride']
    boxes, valid = _geometry(sp, sp['seed'])
    rng = np.random.default_rng(sp['seed'] + 77)
    labels, kps = [], []
    for b in range(B):
        G = sp['n_gt'][b]
        lab = rng.integers(1, C + 1, G)
        if sp['labels'] == 'with_C':
            lab[0] = C
        labels.append(lab.astype(np.int64))
        xy = np.stack([rng.uniform(0, W * s, (G, K)), rng.uniform(0, H * s, (G, K))], 2)
        mode = sp['vis']
        if mode == 'none_and_all':
            mode = 'none' if b == 0 else 'all'
        if mode == 'all':
            v = np.ones((G, K))
        elif mode == 'none':
            v = np.zeros((G, K))
        elif mode == 'values_1_2':
            v = (rng.random((G, K)) < 0.3) * rng.integers(1, 3, (G, K))
        else:                                                       # 'sparse': as the data set marks them, 2 = visible
            v = (rng.random((G, K)) < 0.15) * 2.0
            v[-1] = 0                                               # a gt without a visible keypoint
            if G > 1:
                v[0, 0] = 2.0
        kps.append(np.concatenate([xy, v[:, :, None]], 2).astype(f32))
    case = Case(name=name, regime=sp['regime'], B=B, H=H, W=W, C=C, K=K, stride=float(s), boxes=boxes, valid=valid,
                labels=None if sp['labels'] is None else labels, kps=kps, pos_num=sp['pos_num'],
                normalize_term=float(sp['base_scale'] * s), maps=None, **sp['cfg'])
    if with_maps:
        case.maps = _maps(case, sp, rng)
    return case


def _maps(case, sp, rng):
    """the nine prediction maps: logits ~ 2 randn; offsets such that the decoded coordinates scatter a cell or so around the
    targets' range (raw ~ 4 randn: pred = raw * stride + centre)"""
    B, H, W, C, K = case.B, case.H, case.W, case.C, case.K
    values = sp['values']
    scale = {'1e3': 1e3, 'kink': 1e-3}.get(values, 4.0)

    def mk(ch, sc):
        return (rng.standard_normal((B, ch, H, W), dtype=f32) * f32(sc)).astype(f32)
    maps = dict(cls=[mk(C, 2.0) for _ in range(3)], bbox=[mk(4, scale) for _ in range(3)], kpt=[mk(2 * K, scale) for _ in range(3)])
    if values == 'saturated':       # +-30 and +-100 in every class of a few points, positives and negatives alike
        for s in range(3):
            flat = maps['cls'][s].reshape(B, C, -1)
            for j, v in enumerate((30.0, -30.0, 100.0, -100.0)):
                flat[:, :, j::8] = v
    if values == 'kink':
        # stage 1 boxes: |x| = |pred - target| / normalize_term within an ulp or two of beta at every point and channel, for
        # whatever gt the point is assigned to -- of the FIRST gt here (positives of the others sit away from the kink)
        px, py = grid_points(case.stride, H, W)
        centre = np.stack([px, py, px, py]).astype(f64)
        beta, nt = f64(f32(case.beta[0])), f64(f32(case.normalize_term))
        for b in range(B):
            t = np.asarray(case.boxes[b], f64)[0][:, None]
            sign = np.where(rng.random((4, H * W)) < 0.5, -1.0, 1.0)
            raw = (t + sign * beta * nt - centre) / case.stride
            maps['bbox'][0][b] = raw.astype(f32).reshape(4, H, W)
    return maps
