"""Deformable PS-RoI pooling inputs that sit ON the edges of csrc/psroi.hip (plain numpy + the CPU oracle, no GPU).

The sampling rule of the reference is ``w < -0.5 || w > W - 0.5`` -> skip (both boundaries are INSIDE), then a clamp to
[0, W-1], then floor / ceil corners that coincide on the lattice.  Random RoIs and normal offsets land on -0.5, on W - 0.5 or on
an integer with probability zero, so `>` against `>=` or a wrong clamp cannot be told apart by them.  The table below also walks
the launcher's code paths (kgdet_deform_psroi_forward / _backward) on the smallest shapes that still reach each of them.

A case is a ``Case`` tuple: B, C, H, W, R, out_dim, group_size, pooled_size (P), part_size, sample_per_part (S), num_classes,
no_trans, trans_std, its family and the committed seed.  spatial_scale is 1/16 everywhere.

Families
  exact     P and S are powers of two, RoI corners are even integers with x2 + 1 - x1 a multiple of 16 (the RoI is a whole number
            of map cells wide), offsets are multiples of 1/8 and trans_std is a power of two (or 0).  Every sample coordinate is then
            a dyadic rational below 2^7 with at most 10 fractional bits: exact in float32, so the float32 kernels and the float64
            oracle see the SAME positions and every element is compared with no allowance.  With trans_std = 2^-7 an offset step of
            1/8 moves a sample of a one-cell RoI by 2^-10, and a share of the offset cells is aimed at the palette of ``palette()``:
            exactly -0.5 and L - 0.5, a hair (2^-10) outside each, the two clamp zones, lattice points, cell interiors, far outside.
            The exact cases WITHOUT a fine offset step (no_trans, trans_std 0 or 1) cannot reach the two hair positions -- their
            coordinates are multiples of 1/16 at the finest -- and reach the other classes through crafted RoIs / coarse offsets
            (``possible_classes``).
  general   any P and S, random real RoIs (mostly inside the map, some across its border), normal offsets, trans_std 0.1; RoI 0 is
            the whole map, RoI 1 has width 0 after rounding (the fmax(..., 0.1) branch).  The committed seed is one for which the
            float32 and the float64 oracle agree on `count` in EVERY bin (tests/test_psroi_edge_cases.py asserts it).
  handover  the list-length hand-overs of the grad_data list sorts, see ``handover_rois``.

RoIs whose batch index is outside [0, B) cannot go through the oracle (it would read out of bounds): the reference is computed
without them, their rows of out / count / grad_trans are zero by definition and they add nothing to grad_data.
"""
import collections
import functools

import numpy as np

import oracle

SCALE = 1.0 / 16
E = 2.0 ** -10
T7 = 2.0 ** -7

Case = collections.namedtuple('Case', 'name family B C H W R out_dim group_size pooled_size part_size sample_per_part '
                                      'num_classes no_trans trans_std seed')

HANDOVER_LENGTHS = (64, 65, 256, 257, 512, 513, 1024, 1025, 8192, 8193)

CASES = [
    #    name            family     B    C  H   W   R   od  G   P part S cls no_trans std seed
    # baseline: vec4 lists (4 channels per class), psroi_grad_data<4> (64 records)
    Case('base',         'exact',   2,   8, 6,  7, 12,   8, 1,  4, 4, 2, 2, False, T7, 1),
    # 3 channels per class: psroi_grad_data_lists<1>
    Case('lists1',       'exact',   2,   6, 6,  7, 12,   6, 1,  4, 4, 2, 2, False, T7, 2),
    # 70 per class: forward chunks 64 + 6, psroi_gather<1> second `cc` round with idle lanes, lists<1> with two chunks, three
    # channel tiles (64, 64, 12) of psroi_to_cell_major / psroi_quotient_t
    Case('ch70',         'exact',   2, 140, 5,  6,  8, 140, 1,  4, 4, 2, 2, False, T7, 3),
    # 264 per class: vec4 lists with two 256-channel chunks, the second 8 channels live
    Case('ch264',        'exact',   2, 264, 4,  5,  8, 264, 1,  4, 4, 2, 1, False, T7, 4),
    # C > out_dim * G^2: psroi_zero_tail / the inactive channels of the tile route; one channel per class
    Case('ctail',        'exact',   2,  11, 6,  7, 12,   2, 2,  4, 4, 2, 2, False, T7, 5),
    # PP = 256: four psroi_quotient_t passes, all 256 hit bits, psroi_grad_data<32>, the largest forward LDS
    Case('pp256',        'exact',   2,  32, 6,  7,  6,   2, 4, 16, 8, 2, 1, False, T7, 6),
    # 1024 records at S = 4
    Case('rec1024',      'exact',   2,  16, 6,  7,  6,   4, 2,  8, 4, 4, 2, False, T7, 7),
    # W == 2: both clamp zones next to each other
    Case('w2',           'exact',   2,   8, 5,  2, 12,   8, 1,  4, 4, 2, 2, False, T7, 8),
    # trans_std 0 with offsets present (they must not matter, grad_trans exactly 0); trans_std 1
    Case('tstd0',        'exact',   2,   8, 6,  7, 14,   8, 1,  4, 4, 2, 2, False, 0.0, 9),
    Case('tstd1',        'exact',   2,   8, 6,  7, 14,   8, 1,  4, 4, 2, 2, False, 1.0, 10),
    Case('notrans_x',    'exact',   2,   8, 6,  7, 14,   8, 1,  4, 4, 2, 1, True, 0.0, 11),
    # production geometry, position-sensitive 7x7 groups: psroi_grad_data<13> (784 records)
    Case('prod',         'general', 2,  98, 9, 12,  8,   2, 7,  7, 7, 4, 1, False, 0.1, 1),
    # S*S = 9: the tail of the four-sample rounds; part_size > P: offset cells that own no bin
    Case('s3part7',      'general', 2,   4, 7,  9, 10,   4, 1,  3, 7, 3, 2, False, 0.1, 2),
    # PP = 81: the second b0 pass of psroi_quotient_t, partial
    Case('pp81',         'general', 2,  18, 7,  9,  8,   2, 3,  9, 9, 3, 1, False, 0.1, 3),
    # group_size > P: group cells that own no bin; S*S = 1
    Case('g7s1',         'general', 2,  98, 7,  9, 12,   2, 7,  3, 3, 1, 2, False, 0.1, 4),
    # the record table just under its cap of 2048
    Case('rec2025',      'general', 2,   2, 7,  9,  6,   2, 1,  5, 5, 9, 1, False, 0.1, 5),
    Case('rec1936',      'general', 2,   2, 7,  9,  6,   2, 1, 11, 11, 4, 2, False, 0.1, 6),
    Case('minimal',      'general', 2,   2, 5,  6, 16,   2, 1,  1, 1, 1, 1, False, 0.1, 7),
    # degenerate maps
    Case('map1x1',       'general', 2,   4, 1,  1, 12,   4, 1,  3, 3, 2, 2, False, 0.1, 8),
    Case('map9x15',      'general', 2,   4, 9, 15, 12,   4, 1,  4, 4, 3, 2, False, 0.1, 9),
    # one class per output channel: a 64-channel chunk of the tile route spans three classes
    Case('cls3',         'general', 2,   3, 6,  7, 10,   3, 1,  3, 3, 2, 3, False, 0.1, 10),
    Case('notrans_g',    'general', 2,   4, 6,  7, 10,   4, 1,  7, 7, 3, 1, True, 0.0, 11),
    # images 0 and 2 own no RoI; RoI 2 has batch index -1, RoI 3 has batch index B
    Case('noroi',        'general', 3,   4, 6,  7, 10,   4, 1,  4, 4, 2, 2, False, 0.1, 12),
    # list lengths on both sides of every sort hand-over; R = 20 101 = five list_cap segments of the tile route
    Case('handover',     'handover', 10,  4, 3,  3, sum(HANDOVER_LENGTHS), 4, 1, 1, 1, 1, 1, True, 0.0, 13),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

CLASSES = ('on_lo', 'on_hi', 'hair_lo', 'hair_hi', 'clamp_lo', 'clamp_hi', 'lattice', 'inside', 'far')


def case_id(case):
    return case.name


def classes_of(case):
    """offset classes the kernels see"""
    return 1 if case.no_trans else case.num_classes


def fine_offsets(case):
    """an offset step of 1/8 moves a sample by 2^-10 of a one-cell RoI: the palette, hairs included, is reachable through offsets"""
    return case.family == 'exact' and not case.no_trans and 0.0 < case.trans_std <= T7


def possible_classes(case):
    """the position classes an exact case can produce (module docstring)"""
    return set(CLASSES) if fine_offsets(case) else set(CLASSES) - {'hair_lo', 'hair_hi'}


def palette(L):
    """(targets, weights) of one axis of length L"""
    mid = (L - 1) // 2
    vals = [-0.5, L - 0.5, -0.5 - E, L - 0.5 + E, -0.25, L - 0.75, 0, L - 1, mid, mid + 0.375, 0.625, -40, L + 40]
    wts = [2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 0.5, 0.5]
    if L == 1:       # no open interval (0, L-1): the interior targets become lattice targets
        vals[9], vals[10] = 0, 0
    return np.asarray(vals, np.float64), np.asarray(wts, np.float64) / sum(wts)


def bin_maps(case, dtype=np.float64):
    """(part_of, group_of): offset cell and group cell of every bin row / column, in the arithmetic of `dtype`
    (deform_pool_cuda_kernel.cu:99-106)"""
    T = np.dtype(dtype).type
    ar = np.arange(case.pooled_size).astype(dtype)
    part_of = np.floor(ar / T(case.pooled_size) * T(case.part_size)).astype(np.int64)
    group_of = np.clip(np.floor(ar * T(case.group_size) / T(case.pooled_size)).astype(np.int64), 0, case.group_size - 1)
    return part_of, group_of


def geometry(case, rois, dtype=np.float64):
    """(lo, ext, binsz, sub), each [R, 2] as (x, y): RoI start, clamped extent, bin and sub-bin size on the map (:76-97)"""
    T = np.dtype(dtype).type
    r = rois[:, 1:].astype(dtype)
    rnd = np.sign(r) * np.floor(np.abs(r) + T(0.5))                 # C's round(): half away from zero
    lo = ((rnd[:, :2] * T(SCALE)).astype(np.float64) - 0.5).astype(dtype)
    hi = (((rnd[:, 2:] + T(1)) * T(SCALE)).astype(np.float64) - 0.5).astype(dtype)
    ext = np.maximum((hi - lo).astype(np.float64), 0.1).astype(dtype)
    binsz = ext / T(case.pooled_size)
    sub = binsz / T(case.sample_per_part)
    return lo, ext, binsz, sub


def positions(case, rois, offset, dtype=np.float64):
    """(w [R, classes, P, P, S], h [R, classes, P, P, S]): sample columns (over iw) and rows (over ih) of every bin (ph, pw), in
    the arithmetic of `dtype`, the way the kernels (float32) / the float64 oracle evaluate them (:99-124)"""
    T = np.dtype(dtype).type
    P, S, part, R, ncls = case.pooled_size, case.sample_per_part, case.part_size, rois.shape[0], classes_of(case)
    lo, ext, binsz, sub = geometry(case, rois, dtype)
    part_of, _ = bin_maps(case, dtype)
    if case.no_trans:
        t = np.zeros((R, 1, 2, P, P), dtype)
    else:
        o = offset.astype(dtype).reshape(R, ncls, 2, part, part)
        t = o[:, :, :, part_of][:, :, :, :, part_of] * T(case.trans_std)          # [R, classes, 2, P(ph), P(pw)]
    ar = np.arange(P).astype(dtype)
    col = lambda a: a.reshape(R, 1, 1, 1)
    wstart = ar.reshape(1, 1, 1, P) * col(binsz[:, 0]) + col(lo[:, 0])
    wstart = wstart + t[:, :, 0] * col(ext[:, 0])
    hstart = ar.reshape(1, 1, P, 1) * col(binsz[:, 1]) + col(lo[:, 1])
    hstart = hstart + t[:, :, 1] * col(ext[:, 1])
    s = np.arange(S).astype(dtype)
    w = wstart[..., None] + s * sub[:, 0].reshape(R, 1, 1, 1, 1)
    h = hstart[..., None] + s * sub[:, 1].reshape(R, 1, 1, 1, 1)
    assert w.dtype == np.dtype(dtype) and h.dtype == np.dtype(dtype)
    return w, h


def sample_alive(case, w, h):
    """[R, classes, P, P, S(ih), S(iw)]: the sample is averaged (the boundaries -0.5 and L - 0.5 are inside)"""
    okw = (w >= -0.5) & (w <= case.W - 0.5)
    okh = (h >= -0.5) & (h <= case.H - 0.5)
    return okh[..., :, None] & okw[..., None, :]


def classify_axis(pos, L):
    """{class: number of sample coordinates} of one axis of length L"""
    pos = np.asarray(pos, np.float64)
    whole = pos == np.floor(pos)
    return {
        'on_lo': int((pos == -0.5).sum()),
        'on_hi': int((pos == L - 0.5).sum()),
        'hair_lo': int((pos == -0.5 - E).sum()),
        'hair_hi': int((pos == L - 0.5 + E).sum()),
        'clamp_lo': int(((pos > -0.5) & (pos < 0)).sum()),
        'clamp_hi': int(((pos > L - 1) & (pos < L - 0.5)).sum()),
        'lattice': int((whole & (pos >= 0) & (pos <= L - 1)).sum()),
        'inside': int((~whole & (pos > 0) & (pos < L - 1)).sum()),
        'far': int(((pos < -2) | (pos > L + 1)).sum()),
    }


def valid_rows(case, rois):
    b = rois[:, 0].astype(np.int64)
    return (b >= 0) & (b < case.B)


def classify(case, rois, offset):
    """{'x': {class: count}, 'y': {class: count}} over the samples of the RoIs with a valid batch index (float64 positions)"""
    ok = valid_rows(case, rois)
    w, h = positions(case, rois[ok], None if case.no_trans else offset[ok], np.float64)
    return {'x': classify_axis(w, case.W), 'y': classify_axis(h, case.H)}


def list_lengths(case, rois, offset):
    """[B, classes, G*G, H, W]: entries of every grad_data contribution list = corners of alive samples that land on the pixel
    (one entry per corner, coinciding corners included), from the float64 positions"""
    ok = valid_rows(case, rois)
    rois = rois[ok]
    w, h = positions(case, rois, None if case.no_trans else offset[ok], np.float64)
    alive = sample_alive(case, w, h)
    wc, hc = np.clip(w, 0, case.W - 1), np.clip(h, 0, case.H - 1)
    G, P = case.group_size, case.pooled_size
    _, group_of = bin_maps(case)
    out = np.zeros((case.B, classes_of(case), G * G, case.H, case.W), np.int64)
    shape = alive.shape
    n, cls, ph, pw, ih, iw = np.nonzero(alive)
    b = rois[:, 0].astype(np.int64)[n]
    k = group_of[ph] * G + group_of[pw]
    xs, ys = wc[n, cls, ph, pw, iw], hc[n, cls, ph, pw, ih]
    assert shape[0] == rois.shape[0]
    for y in (np.floor(ys), np.ceil(ys)):
        for x in (np.floor(xs), np.ceil(xs)):
            np.add.at(out, (b, cls, k, y.astype(np.int64), x.astype(np.int64)), 1)
    return out


def empty_offset_cells(case):
    """[part, part] bool: offset cells that own no bin (part_size > pooled_size): grad_trans is exactly 0 there"""
    part_of, _ = bin_maps(case)
    owned = np.zeros(case.part_size, bool)
    owned[part_of] = True
    return ~(owned[:, None] & owned[None, :])


def empty_group_channels(case):
    """[C] bool: input channels whose group cell owns no bin (group_size > pooled_size) or that lie beyond out_dim * G^2:
    grad_data is exactly 0 there"""
    _, group_of = bin_maps(case)
    G = case.group_size
    owned = np.zeros(G, bool)
    owned[group_of] = True
    cell = (owned[:, None] & owned[None, :]).reshape(-1)
    c = np.arange(case.C)
    return (c >= case.out_dim * G * G) | ~cell[c % (G * G)]


# ------------------------------------------------------------------------------------------------------------------ generators
def exact_rois(case, rng):
    """even integer corners, x2 + 1 - x1 = 16 k (k = 1 .. 3 map cells), mostly inside the map"""
    R = case.R
    rois = np.empty((R, 5), np.float64)
    rois[:, 0] = rng.integers(0, case.B, R)
    for axis, L in enumerate((case.W, case.H)):
        k = rng.integers(1, min(L, 3) + 1, R)
        x1 = 2 * rng.integers(-4, 8 * L - 8 * k + 5)                # in [-8, 16 (L - k) + 8]
        rois[:, 1 + axis] = x1
        rois[:, 3 + axis] = x1 + 16 * k - 1
    if not fine_offsets(case) and (case.no_trans or case.trans_std == 0.0):
        # no offsets to aim with: one-cell RoIs whose samples (multiples of 1/8 from the RoI start at P 4, S 2) sit on the palette
        for i, (fx, fy) in enumerate(_crafted_starts(case.W, case.H)):
            rois[i, 1:] = [fx, fy, fx + 15, fy + 15]
    return rois.astype(np.float32)


def _crafted_starts(W, H):
    """(x1, y1) of six one-cell RoIs: first sample on -0.5; a sample on L - 0.5; in [-0.5, 0); in (L-1, L-0.5); on an interior
    lattice point; far outside (the other axis inside the map)"""
    def axis(L):
        m = (L - 1) // 2
        return [0, 16 * (L - 1) + 8, 4, 16 * (L - 1) + 12, 8 + 16 * m, 16 * L + 48]
    xs, ys = axis(W), axis(H)
    inside_x, inside_y = 8 + 16 * ((W - 1) // 2) + 4, 8 + 16 * ((H - 1) // 2) + 4
    return [(xs[i], ys[i]) for i in range(5)] + [(xs[5], inside_y), (inside_x, ys[5])]


def exact_offsets(case, rois, rng, edge_share=0.6):
    """float32 [R, 2 * classes, part, part], multiples of 1/8.  Free cells: a shift of about a quarter of the RoI.  With
    trans_std > 0 a share `edge_share` of the cells that own a bin aims one sample of their first bin at a palette position"""
    R, ncls, part, S = case.R, case.num_classes, case.part_size, case.sample_per_part
    ts = case.trans_std
    step = ts if ts > 0 else 1.0
    off = np.round(rng.standard_normal((R, ncls, 2, part, part)) * 0.25 / step * 8) / 8
    if ts > 0:
        lo, ext, binsz, sub = geometry(case, rois)
        part_of, _ = bin_maps(case)
        first_bin = {int(q): int(np.nonzero(part_of == q)[0][0]) for q in np.unique(part_of)}
        for axis, L in enumerate((case.W, case.H)):
            vals, wts = palette(L)
            for q, p in first_bin.items():
                # x offsets of cell column q (every cell row), y offsets of cell row q (every cell column)
                shape = (R, ncls, part)
                aim = rng.random(shape) < edge_share
                target = vals[rng.choice(len(vals), size=shape, p=wts)]
                i = rng.integers(0, S, shape)
                base = p * binsz[:, axis].reshape(R, 1, 1) + lo[:, axis].reshape(R, 1, 1) + i * sub[:, axis].reshape(R, 1, 1)
                aimed = np.round((target - base) / (ts * ext[:, axis].reshape(R, 1, 1)) * 8) / 8
                if axis == 0:
                    off[:, :, 0, :, q] = np.where(aim, aimed, off[:, :, 0, :, q])
                else:
                    off[:, :, 1, q, :] = np.where(aim, aimed, off[:, :, 1, q, :])
    out = off.reshape(R, 2 * ncls, part, part).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), off.reshape(out.shape))
    return out


def general_rois(case, rng):
    """random real corners, mostly inside the map, some across its border; RoI 0 the whole map, RoI 1 of width 0 after rounding"""
    R = case.R
    rois = np.empty((R, 5), np.float64)
    rois[:, 0] = rng.integers(0, case.B, R)
    for axis, L in enumerate((case.W, case.H)):
        px = 16.0 * L
        x1 = rng.uniform(-0.15 * px, 0.7 * px, R)
        rois[:, 1 + axis] = x1
        rois[:, 3 + axis] = x1 + rng.uniform(0.15, 0.9, R) * px
    rois[0, 1:] = [0, 0, 16 * case.W - 1, 16 * case.H - 1]
    cx, cy = 16 * case.W * 0.4, 16 * case.H * 0.6
    rois[1, 1:] = [round(cx) + 0.1, round(cy) - 0.2, round(cx) + 0.4, round(cy) + 0.3]
    return rois.astype(np.float32)


def handover_rois(case):
    """P 1, S 1, no_trans: the one sample of the RoI (20, 12, 35, 27) lies at (0.75, 0.25), strictly inside the cell of pixels
    (0..1, 0..1); k_b copies on image b put exactly k_b entries on each of that image's four corner lists"""
    rows = [np.tile(np.array([[b, 20, 12, 35, 27]], np.float32), (k, 1)) for b, k in enumerate(HANDOVER_LENGTHS)]
    return np.concatenate(rows)


def inputs(case):
    """dict(data, rois, offset (None with no_trans), grad_out), float32, from the case's committed seed"""
    rng = np.random.default_rng(1000 + case.seed)
    c = case
    data = rng.standard_normal((c.B, c.C, c.H, c.W)).astype(np.float32)
    grad_out = rng.standard_normal((c.R, c.out_dim, c.pooled_size, c.pooled_size)).astype(np.float32)
    if c.family == 'handover':
        rois, offset = handover_rois(c), None
    elif c.family == 'exact':
        rois = exact_rois(c, rng)
        offset = None if c.no_trans else exact_offsets(c, rois, rng)
    else:
        rois = general_rois(c, rng)
        offset = None if c.no_trans else (rng.standard_normal((c.R, 2 * c.num_classes, c.part_size, c.part_size)) *
                                          0.5).astype(np.float32)
    if c.name == 'noroi':
        rois[:, 0] = 1
        rois[2, 0], rois[3, 0] = -1, c.B
    assert rois.shape == (c.R, 5)
    return dict(data=data, rois=rois, offset=offset, grad_out=grad_out)


def _oracle(case, inp, dtype):
    """the oracle's forward and backward in `dtype` over the RoIs with a valid batch index, rows of the others zero"""
    c = case
    ok = valid_rows(c, inp['rois'])
    rows = lambda a: None if a is None else np.ascontiguousarray(a[ok], dtype)
    T = np.dtype(dtype).type
    data, rois, offset, go = inp['data'].astype(dtype), rows(inp['rois']), rows(inp['offset']), rows(inp['grad_out'])
    args = (T(SCALE), c.pooled_size, c.out_dim, c.no_trans, c.group_size, c.part_size, c.sample_per_part, T(c.trans_std))
    out_v, cnt_v = oracle.deform_psroi_forward(data, rois, offset, *args)
    gd, gt_v = oracle.deform_psroi_backward(go, cnt_v, data, rois, offset, *args)
    out = np.zeros((c.R,) + out_v.shape[1:], dtype)
    count = np.zeros_like(out)
    out[ok], count[ok] = out_v, cnt_v
    gt = None
    if not c.no_trans:
        gt = np.zeros(inp['offset'].shape, dtype)
        gt[ok] = gt_v
    return out, count, gd, gt


@functools.lru_cache(maxsize=None)
def reference(case):
    """inputs + the float64 oracle's out, count, grad_data, grad_trans + the float32 oracle's out32, count32, grad_data32,
    grad_trans32 (the serial float32 evaluation grad_data is held to bit for bit).  Computed once per case, read-only."""
    inp = inputs(case)
    res = dict(inp)
    res['out'], res['count'], res['grad_data'], res['grad_trans'] = _oracle(case, inp, np.float64)
    res['out32'], res['count32'], res['grad_data32'], res['grad_trans32'] = _oracle(case, inp, np.float32)
    for a in res.values():
        if a is not None:
            a.setflags(write=False)
    return res


def bar(ref32, ref64):
    """(scale, bar) of one quantity of one case: 4 x the float32 oracle's own distance from the float64 oracle, as a fraction of the
    float64 result's scale, never below 8 x 2^-24.  The kernels form the float32 oracle's products and add them in another order
    (four-sample rounds, 64-lane butterfly, bins folded into offset cells): the factor covers order, not wrong terms."""
    scale = max(float(np.abs(ref64).max()), 1e-6)
    own = float(np.abs(ref32.astype(np.float64) - ref64).max()) / scale
    return scale, max(4.0 * own, 8.0 * 2.0 ** -24)
