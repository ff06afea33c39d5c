"""Cases and plain numpy references for ``kgdet_aug_merge`` (csrc/aug_merge.hip), shared by tests/test_aug_merge_refs.py (CPU:
the references held to each other and to ``detector.merge_aug_results_kp``) and tests/test_gpu_aug_merge.py (the kernel through
the C ABI).  No torch here.

One operation, stated twice:

* ``reference_f32``: the arithmetic of include/kgdet_hip.h, every operation rounded to float32 in the order written --
  flipped x = ``(float32(w) - x) - float32(1)``, x1 / x2 of a box swapped, landmarks GATHERED (``k[:, perm]``: out slot k takes
  input slot perm[k]), then box coordinates and landmark x, y times ``float32(1.0 / s)``; visibility and scores copied bit for
  bit.  The kernel must give these bits.
* ``reference_f64``: the same mapping in float64 with a true division by s, and the bound a float32 evaluation may be off by.
  With U = 2^-24 (half an ulp, the relative error of one float32 rounding in the normal range):
    unflipped:  |x rn(1/s) - x/s| <= U |ref| (reciprocal) + U |ref| (1 + U) (product)      -> 2U |ref| (1 + 4U)
    flipped x:  rn(w - x) is off by <= U |w - x|, rn(. - 1) by <= U |w - x - 1| (1 + U); both are scaled by 1/s and go through
                the two roundings above                                    -> (2U |ref| + U (|w - x| + |w - x - 1|) / s) (1 + 4U)
  The (1 + 4U) takes the second-order terms.  The count assumes relative roundings, so ``bound_mask`` leaves out what float32
  cannot hold that way: results beyond its largest finite value or below its smallest normal one, and non-finite references.
  Those elements are still held to the bits of ``reference_f32``.

Path notes (kTileRows = 8 rows per workgroup, 8192 floats of LDS per chunk, 256 threads):
  K = 1     3 floats per row: shorter than one dwordx4; heads of 0 .. 3 floats as the rows go
  K = 5     15 floats per row: row starts fall on every residue of 16 bytes -> source and destination heads of 1, 2, 3 floats
  K = 21    63 floats per row, one chunk
  K = 294   882 floats per row (3528 bytes = 8 mod 16): 8 rows per chunk, one trip; heads 0 / 2, with an odd base offset 1 / 3
  K = 342   1026 floats per row: 7 rows fit, a tile of 8 takes a second trip (7 + 1)
  K = 683   2049 floats per row: 3 + 3 + 2
  K = 1024  3072 floats per row: 2 rows x 4 trips, and the permutation load strides over the 256 threads four times
  rows 0 / 1 / 7 / 8 / 9 / 17 per augmentation: no tile, a tile of 1, one short of a tile, a full tile, one and two full tiles + 1
"""
import types
import zlib

import numpy as np

U = 2.0 ** -24
F32_MAX = float(np.finfo(np.float32).max)
F32_TINY = float(np.finfo(np.float32).tiny)          # smallest normal
MAX_K, MAX_SEGS = 1024, 16

SCALES = [1.6660, 1.2495, 2.0, 0.75, 1.0 / 3.0, 1e-3, 1e3]
WIDTHS = [1.0, 999.0, 1333.0]


def _bits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


# what a copy must carry through: quiet and signalling NaNs with payloads, both infinities, -0.0, subnormals
COPIED_SPECIALS = _bits(0x7fc01234, 0xffc00001, 0x7f800001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff, 0x00400000)


def demo_perm():
    """the DeepFashion2 left/right involution over the 294 landmarks (datasets.landmark_fields)"""
    from kgdet_amd.evaluation import landmark_meta
    perm = np.arange(294)
    for pairs in landmark_meta()['swap_pairs']:
        for a, b in pairs:
            perm[a], perm[b] = b, a
    return perm.astype(np.int32)


def make_perm(kind, K):
    if kind is None:
        return None
    if kind == 'demo':
        assert K == 294
        return demo_perm()
    if kind == 'identity':
        return np.arange(K, dtype=np.int32)
    if kind == 'reverse':                       # an involution for any K
        return np.arange(K - 1, -1, -1, dtype=np.int32)
    if kind == 'cycle3':                        # NOT an involution: out slots 0, 1, 2 take input slots 1, 2, 0
        assert K >= 3
        p = np.arange(K, dtype=np.int32)
        p[:3] = [1, 2, 0]
        return p
    raise KeyError(kind)


def flip_indices_of(perm):
    """``flip_indices`` over interleaved (x, y) channels whose ``[0::2] // 2`` is ``perm`` (datasets.landmark_fields)"""
    perm = np.asarray(perm, dtype=np.int64)
    return np.stack([perm * 2, perm * 2 + 1], axis=1).reshape(-1)


def _segs(rows, flips=None, w=999.0, s=1.2495):
    flips = flips if flips is not None else [i % 2 == 0 for i in range(len(rows))]
    return [(n, w, s, f) for n, f in zip(rows, flips)]


def _table():
    t = {}

    def add(name, K, segs, perm='auto', S=14, offsets=(0, 0), values='plain'):
        """segs: [(rows, img_w, scale, flip)]; offsets: (first source landmark offset, out_kpts offset) in floats past a 16-byte
        boundary -- the source offset advances by one float per augmentation"""
        if perm == 'auto':
            perm = 'demo' if K == 294 else 'reverse'
        t[name] = dict(K=K, S=S, segs=list(segs), perm=perm, offsets=offsets, values=values)

    for K in (1, 5, 21, 294, 342, 683, 1024):                                   # 9 = a full tile (every chunk trip) + a tile of 1
        add('K%d' % K, K, [(9, 999.0, 1.2495, True), (8, 1333.0, 1.6660, False), (1, 999.0, 0.75, True)])
    for K in (5, 294, 342):
        add('rows_K%d' % K, K, _segs([0, 1, 7, 8, 9, 17]))
        add('rows_K%d_other_flips' % K, K, _segs([17, 9, 8, 7, 1, 0]))
    add('A1', 21, _segs([9]))
    for K in (5, 21):                                                          # empty augmentations first, in the middle, last
        add('A16_K%d' % K, K, _segs([0, 3, 0, 0, 9, 1, 8, 0, 17, 2, 0, 7, 1, 5, 4, 0], flips=[i % 3 != 1 for i in range(16)]))
    add('S1', 21, _segs([9, 1, 8]), S=1)
    add('S15', 21, _segs([9, 1, 8]), S=15)
    for K in (1, 5, 294):
        for off in range(4):
            add('off%d_K%d' % (off, K), K, _segs([3, 9, 1, 2]), offsets=(off, off))
        add('off_src1_out3_K%d' % K, K, _segs([3, 9, 1, 2]), offsets=(1, 3))
    add('perm_demo', 294, _segs([3, 2], flips=[True, True]), perm='demo')
    add('perm_identity', 294, _segs([3, 2], flips=[True, True]), perm='identity')
    for K in (5, 294, 1024):
        add('perm_cycle3_K%d' % K, K, _segs([9, 2], flips=[True, True]), perm='cycle3')
    add('noflip_null_perm', 21, _segs([9, 1], flips=[False, False]), perm=None)
    add('flipped_but_empty_null_perm', 21, _segs([0, 9, 0], flips=[True, False, True]), perm=None)
    for w in WIDTHS:                                                            # 7 scales x (flip, no flip) = 14 augmentations
        add('scales_w%d' % w, 21, [(3, w, s, f) for s in SCALES for f in (True, False)], values='edges')
        add('scales_w%d_K5' % w, 5, [(9, w, s, f) for s in SCALES for f in (False, True)], values='edges', offsets=(1, 3))
    add('pow2_scales', 21, [(4, w, s, f) for w in WIDTHS for s in (0.5, 1.0, 2.0) for f in (True, )]
        + [(4, 999.0, s, False) for s in (0.5, 1.0, 2.0)], values='edges')
    add('nonfinite_copied', 21, _segs([9, 8, 1]), values='nonfinite')
    add('nonfinite_copied_K294', 294, _segs([2, 9]), values='nonfinite', offsets=(3, 1))
    return t


TABLE = _table()
NAMES = list(TABLE)
TORCH_EXACT_SCALES = (0.5, 1.0, 2.0)        # 1/s exact in float32: x * (1/s) IS x / s


def _edge_values(w):
    return np.array([0.0, w / 2, w, w + 0.5, 2 * w + 3, 1e30, -1e30, -0.0, 1e-40, -1e-42, w - 1, 1.0, 0.5 * w + 0.25],
                    dtype=np.float32)


def case(name):
    """the inputs of one launch: K, S, perm (int32 [K] or None), segs = [namespace(boxes [n,4], scores [n,S], kpts [n,K,3],
    n, w, s, flip)], offsets"""
    spec = TABLE[name]
    K, S = spec['K'], spec['S']
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    segs = []
    for n, w, s, flip in spec['segs']:
        boxes = (rng.random((n, 4)) * 1.2 * w - 5).astype(np.float32)
        scores = rng.random((n, S)).astype(np.float32)
        kpts = (rng.random((n, K, 3)) * np.array([1.2 * w, 900.0, 3.0]) - np.array([3.0, 3.0, 0.5])).astype(np.float32)
        if spec['values'] == 'edges' and n:
            e = _edge_values(w)
            b, k = boxes.reshape(-1), kpts.reshape(-1, 3)
            b[:min(b.size, e.size)] = e[:b.size]
            m = min(k.shape[0], e.size)
            k[:m, 0] = e[:m]                                          # x: every edge value
            k[k.shape[0] - m:, 1] = e[:m][::-1]                        # y likewise (never flipped), from the other end
        if spec['values'] == 'nonfinite' and n:
            v, sc = kpts[..., 2].reshape(-1), scores.reshape(-1)
            m = min(v.size, COPIED_SPECIALS.size)
            v[:m] = COPIED_SPECIALS[:m]
            v[v.size - m:] = COPIED_SPECIALS[:m][::-1]
            m = min(sc.size, COPIED_SPECIALS.size)
            sc[sc.size - m:] = COPIED_SPECIALS[:m]
            kpts[..., 2] = v.reshape(kpts.shape[:2])
            scores = sc.reshape(scores.shape)
        segs.append(types.SimpleNamespace(boxes=boxes, scores=scores, kpts=kpts, n=n, w=float(w), s=float(s), flip=bool(flip)))
    return types.SimpleNamespace(name=name, K=K, S=S, perm=make_perm(spec['perm'], K), perm_kind=spec['perm'], segs=segs,
                                 offsets=spec['offsets'], T=sum(g.n for g in segs))


def reference_f32(c):
    """(boxes [T,4], scores [T,S], kpts [T,K,3]) float32: the header's arithmetic, operation by operation in float32"""
    one = np.float32(1)
    out_b, out_s, out_k = [], [], []
    with np.errstate(all='ignore'):
        for g in c.segs:
            b, k = g.boxes.copy(), g.kpts.copy()
            if g.flip and g.n:                                        # (an empty flipped augmentation needs no permutation)
                w = np.float32(g.w)
                b = np.stack([(w - g.boxes[:, 2]) - one, g.boxes[:, 1], (w - g.boxes[:, 0]) - one, g.boxes[:, 3]], axis=1)
                k = g.kpts[:, c.perm].copy()                          # gather: out slot k takes input slot perm[k]
                k[..., 0] = (w - k[..., 0]) - one
            inv = np.float32(1.0 / g.s)
            b = b * inv
            k[..., :2] = k[..., :2] * inv
            assert b.dtype == np.float32 and k.dtype == np.float32
            out_b.append(b); out_s.append(g.scores.copy()); out_k.append(k)
    return (np.concatenate(out_b).reshape(-1, 4), np.concatenate(out_s).reshape(-1, c.S), np.concatenate(out_k).reshape(-1, c.K, 3))


def reference_f64(c):
    """(boxes, kpts, bound_boxes, bound_kpts) float64: the mapping with a true division, and the counted bound per element
    (module docstring); the bound of a visibility is 0 -- it is a copy"""
    out = [[], [], [], []]
    with np.errstate(all='ignore'):
        for g in c.segs:
            b, k = g.boxes.astype(np.float64), g.kpts.astype(np.float64)
            slack_b, slack_k = np.zeros_like(b), np.zeros_like(k)
            if g.flip and g.n:                                        # (an empty flipped augmentation needs no permutation)
                d2, d0 = g.w - b[:, 2], g.w - b[:, 0]
                slack_b[:, 0] = U * (np.abs(d2) + np.abs(d2 - 1)) / g.s
                slack_b[:, 2] = U * (np.abs(d0) + np.abs(d0 - 1)) / g.s
                b = np.stack([d2 - 1, b[:, 1], d0 - 1, b[:, 3]], axis=1)
                k = k[:, c.perm].copy()
                d = g.w - k[..., 0]
                slack_k[..., 0] = U * (np.abs(d) + np.abs(d - 1)) / g.s
                k[..., 0] = d - 1
            b = b / g.s
            k[..., :2] = k[..., :2] / g.s
            bound_k = (2 * U * np.abs(k) + slack_k) * (1 + 4 * U)
            bound_k[..., 2] = 0
            out[0].append(b); out[1].append(k); out[2].append((2 * U * np.abs(b) + slack_b) * (1 + 4 * U)); out[3].append(bound_k)
    return (np.concatenate(out[0]).reshape(-1, 4), np.concatenate(out[1]).reshape(-1, c.K, 3),
            np.concatenate(out[2]).reshape(-1, 4), np.concatenate(out[3]).reshape(-1, c.K, 3))


def bound_mask(ref64):
    """elements the counted bound speaks about: a finite reference that float32 holds as zero or as a normal number"""
    a = np.abs(ref64)
    with np.errstate(invalid='ignore'):
        return np.isfinite(ref64) & (a <= F32_MAX * (1 - 2 * U)) & ((a == 0) | (a >= F32_TINY * (1 + 4 * U)))


def bound_ratio(got, ref64, bound, what=''):
    """max |got - ref64| / bound over ``bound_mask`` (0 / 0 counts as 0), printed; (ratio, elements counted)"""
    mask = bound_mask(ref64)
    if got.shape[-1] == 3:
        mask = mask.copy()
        mask[..., 2] = False                                          # visibility is held to bits, not to a bound
    with np.errstate(all='ignore'):
        err = np.abs(got.astype(np.float64) - ref64)
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(mask, r, 0.0)
    worst = float(r.max()) if r.size else 0.0
    print('%s: error %.3f of its bound over %d of %d elements' % (what, worst, int(mask.sum()), mask.size))
    return worst, int(mask.sum())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def first_difference(a, b):
    """for an assertion message: where two float32 arrays of one shape first differ in bits"""
    x, y = np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1), np.ascontiguousarray(b, np.float32).view(np.uint32).reshape(-1)
    bad = np.nonzero(x != y)[0]
    if not bad.size:
        return 'equal'
    i = int(bad[0])
    return '%d of %d differ, first at flat %d: %08x against %08x' % (bad.size, x.size, i, x[i], y[i])


# refusals: (name, what to break, expected status or None for "any error"); applied to case 'K21' by the GPU test
E_SHAPE, E_UNSUPPORTED = 1, 4
REFUSALS = [
    ('A0', dict(A=0), E_SHAPE),
    ('A17', dict(A=17), E_UNSUPPORTED),
    ('K0', dict(K=0), E_SHAPE),
    ('K1025', dict(K=1025), E_SHAPE),
    ('S0', dict(S=0), E_SHAPE),
    ('negative_n', dict(n=-1), E_SHAPE),
    ('null_boxes', dict(null='boxes'), E_SHAPE),
    ('null_scores', dict(null='scores'), E_SHAPE),
    ('null_kpts', dict(null='kpts'), E_SHAPE),
    ('scale_zero', dict(scale=0.0), E_SHAPE),
    ('scale_negative', dict(scale=-1.5), E_SHAPE),
    ('scale_nan', dict(scale=float('nan')), E_SHAPE),
    ('null_perm_flipped', dict(null='perm'), E_SHAPE),
    ('null_out_kpts', dict(null='out_kpts'), E_SHAPE),
]
