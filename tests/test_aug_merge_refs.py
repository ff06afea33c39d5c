"""tests/aug_merge_cases.py held to its own claims on the CPU: the float32 statement of ``kgdet_aug_merge`` stays inside the
counted bound of the float64 one, equals ``detector.merge_aug_results_kp`` on CPU tensors bit for bit where 1/s is exact
(s = 0.5, 1, 2) and stays within the bound of it elsewhere (CPU torch divides truly, the GPU multiplies by the float32
reciprocal), and gathers."""
import numpy as np
import pytest
import torch

from kgdet_amd.detector import merge_aug_results_kp
from kgdet_amd.postprocess import flip_perm
from tests import aug_merge_cases as M


def _is_involution(perm):
    return perm is None or np.array_equal(perm[perm], np.arange(len(perm)))


def _torch_merge(c):
    """merge_aug_results_kp on CPU tensors -> numpy (boxes, scores, kpts)"""
    fi = M.flip_indices_of(c.perm if c.perm is not None else np.arange(c.K))     # (NULL permutation: only empty flips)
    metas = [dict(img_shape=(800, g.w, 3), scale_factor=g.s, flip=g.flip, flip_indices=fi) for g in c.segs]
    out = merge_aug_results_kp([torch.from_numpy(g.boxes) for g in c.segs], [torch.from_numpy(g.scores) for g in c.segs],
                               [torch.from_numpy(g.kpts) for g in c.segs], metas)
    return [t.numpy() for t in out]


def test_the_table_reaches_what_it_names():
    ks = {M.TABLE[n]['K'] for n in M.NAMES}
    assert {1, 5, 21, 294, 342, 683, 1024} <= ks
    rows = {s[0] for n in M.NAMES for s in M.TABLE[n]['segs']}
    assert {0, 1, 7, 8, 9, 17} <= rows
    assert {M.TABLE[n]['S'] for n in M.NAMES} == {1, 14, 15}
    assert {len(M.TABLE[n]['segs']) for n in M.NAMES} >= {1, 16}
    assert all(len(M.TABLE[n]['segs']) <= M.MAX_SEGS for n in M.NAMES)
    for K in (1, 5, 294):
        assert {M.TABLE['off%d_K%d' % (o, K)]['offsets'] for o in range(4)} == {(o, o) for o in range(4)}
    scales = {s[2] for n in M.NAMES for s in M.TABLE[n]['segs']}
    assert set(M.SCALES) <= scales and set(M.TORCH_EXACT_SCALES) <= scales
    for w in M.WIDTHS:
        assert {(s[2], s[3]) for s in M.TABLE['scales_w%d' % w]['segs']} == {(s, f) for s in M.SCALES for f in (True, False)}
    assert {M.TABLE[n]['perm'] for n in M.NAMES} == {'demo', 'identity', 'reverse', 'cycle3', None}
    # chunk trips of a full tile of 8 rows: 8192 // (3K) rows per trip
    trips = {K: -(-8 // min(8, 8192 // (3 * K))) for K in (294, 342, 683, 1024)}
    assert trips == {294: 1, 342: 2, 683: 3, 1024: 4}
    assert 8192 // (3 * 341) == 8 and 8192 // (3 * 342) == 7                 # 342 is the first K with a second trip
    # K = 5: row starts fall on every residue of 16 bytes; K = 294: only 0 and 8 bytes
    assert {(15 * r * 4) % 16 for r in range(17)} == {0, 4, 8, 12}
    assert {(882 * r * 4) % 16 for r in range(17)} == {0, 8}


def test_demo_perm_is_the_datasets_involution():
    from tests.golden import demo_cases
    fi = demo_cases.demo_dataset(test_mode=True).flip_indices
    p = M.demo_perm()
    assert np.array_equal(np.asarray(fi)[0::2] // 2, p) and _is_involution(p) and (p != np.arange(294)).any()
    assert np.array_equal(flip_perm(M.flip_indices_of(p), 'cpu').numpy(), p)


@pytest.mark.parametrize('name', M.NAMES)
def test_float32_statement_within_the_counted_bound_of_float64(name):
    c = M.case(name)
    b32, s32, k32 = M.reference_f32(c)
    b64, k64, bb, bk = M.reference_f64(c)
    assert b32.shape == (c.T, 4) and s32.shape == (c.T, c.S) and k32.shape == (c.T, c.K, 3)
    rb, nb = M.bound_ratio(b32, b64, bb, name + ' boxes')
    rk, nk = M.bound_ratio(k32, k64, bk, name + ' landmarks')
    assert rb <= 1.0 and rk <= 1.0
    assert nb + nk > 0.5 * (b32.size + 2 * k32.size // 3)           # (the mask leaves out the overflowing edge values only)
    # copies: visibility and scores carry their bits
    assert M.same_bits(s32, np.concatenate([g.scores for g in c.segs]).reshape(-1, c.S))
    vis = np.concatenate([(g.kpts[:, c.perm] if g.flip else g.kpts)[..., 2].reshape(-1) for g in c.segs])
    assert M.same_bits(k32[..., 2].reshape(-1), vis)


@pytest.mark.parametrize('name', M.NAMES)
def test_float32_statement_against_torch_on_the_cpu(name):
    c = M.case(name)
    if not _is_involution(c.perm):
        with pytest.raises(ValueError):
            flip_perm(M.flip_indices_of(c.perm), 'cpu')               # the Python route refuses it: C ABI only
        return
    b32, s32, k32 = M.reference_f32(c)
    tb, ts, tk = _torch_merge(c)
    assert M.same_bits(s32, ts), M.first_difference(s32, ts)
    assert M.same_bits(k32[..., 2], tk[..., 2])
    b64, k64, bb, bk = M.reference_f64(c)
    row = 0
    for g in c.segs:                                                  # per augmentation: exact scales bit for bit
        sl = slice(row, row + g.n)
        row += g.n
        if g.s in M.TORCH_EXACT_SCALES:
            assert M.same_bits(b32[sl], tb[sl]), (g.s, M.first_difference(b32[sl], tb[sl]))
            assert M.same_bits(k32[sl], tk[sl]), (g.s, M.first_difference(k32[sl], tk[sl]))
    # every scale: within the counted bound of the true division.  (Both are float32 numbers, x * rn(1/s) is within 2U |ref| of
    # the quotient and torch's rounding of it within U |ref|: under 1.5 ulp apart, so at most ONE ulp, which is <= 2U |ref|.)
    with np.errstate(all='ignore'):
        ok_b = M.bound_mask(b64) & M.bound_mask(tb.astype(np.float64))
        ok_k = M.bound_mask(k64) & M.bound_mask(tk.astype(np.float64))
        db = np.where(ok_b, np.abs(b32.astype(np.float64) - tb), 0.0)
        dk = np.where(ok_k, np.abs(k32.astype(np.float64) - tk), 0.0)
        rb = np.where(db == 0, 0.0, db / bb)
        rk = np.where(dk == 0, 0.0, dk / bk)
    worst = max(float(rb.max()) if rb.size else 0.0, float(rk[..., :2].max()) if rk.size else 0.0)
    print('%s: float32 statement against CPU torch, %.3f of the bound' % (name, worst))
    assert worst <= 1.0


def test_cpu_torch_divides_truly():
    """the record behind the docstrings: at s = 1.666 a good share of the coordinates differs between x * float32(1/s) and
    CPU torch's x / s, at s = 2 none"""
    c = M.case('scales_w999')
    b32, _, k32 = M.reference_f32(c)
    tb, _, tk = _torch_merge(c)
    row, share = 0, {}
    for g in c.segs:
        a, b = k32[row:row + g.n, :, :2], tk[row:row + g.n, :, :2]
        share.setdefault(g.s, []).append(float((a.view(np.uint32) != b.view(np.uint32)).mean()))
        row += g.n
    print({s: max(v) for s, v in share.items()})
    assert max(share[2.0]) == 0.0
    assert min(share[1.6660]) > 0.05 and min(share[1.0 / 3.0]) > 0.05


def test_landmarks_are_gathered():
    """out slot k takes input slot perm[k].  On the 3-cycle (1, 2, 0) a scatter (input slot k moves to out slot perm[k]) gives
    another answer; on an involution the two coincide, which is why only a non-involution can tell them apart."""
    c = M.case('perm_cycle3_K5')
    assert not _is_involution(c.perm) and list(c.perm[:3]) == [1, 2, 0]
    for g in c.segs:                                                  # mark every slot: y = slot number, visibility = 10 + slot
        g.kpts[..., 1] = np.arange(c.K, dtype=np.float32)[None, :]
        g.kpts[..., 2] = 10 + np.arange(c.K, dtype=np.float32)[None, :]
        g.s = 1.0
    _, _, k32 = M.reference_f32(c)
    _, k64, _, _ = M.reference_f64(c)
    for k in (k32, k64):
        assert (k[:, :, 1] == c.perm[None, :]).all() and (k[:, :, 2] == 10 + c.perm[None, :]).all()
        scattered = np.empty(c.K)
        scattered[c.perm] = np.arange(c.K)
        assert not (k[0, :, 1] == scattered).all()
    inv = M.case('K5')
    assert _is_involution(inv.perm)
    scattered = np.empty(inv.K, np.int64)
    scattered[inv.perm] = np.arange(inv.K)
    assert np.array_equal(scattered, inv.perm)
