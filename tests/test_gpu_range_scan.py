"""kgdet_range_scan_multi (kgdet_amd/csrc/range_scan.hip) through the C ABI against the numpy restatement of its record
(tests/envelope_refs.py): ONE table holds every case -- element counts 1, 3, 5, 63, 64, 65, 4097 and one beyond a row's capped
grid (computed from kgdet_range_scan_blocks / _chunk: the stride loop makes a second trip), base pointers 0, 4, 8 and 12 bytes off
16-byte alignment; zeros, a NaN / +inf / -inf at the first, a middle and the last element, a value AT the limit and one float
above it, subnormals, weights with per-row BatchNorm scales (one running variance of 1e-12).  Counts equal the reference exactly;
the maximum is bit-equal without a row scale and within 4 float32 ulps with one (the square root and the division are the only
operations whose rounding may differ from numpy's).  The records sit between canaries and are pre-filled with 0xFF; the table is
launched twice (a record is overwritten, not accumulated)."""
import ctypes

import numpy as np
import pytest
import torch

from kgdet_amd import _lib
from tests import envelope_refs as ref

pytestmark = pytest.mark.gpu
HI1, HI2 = np.float32(255.875), np.float32(511.75)
SMALL_COUNTS = [1, 3, 5, 63, 64, 65, 4097]


def _lib_scan():
    L = _lib.lib()
    L.kgdet_range_scan_blocks.restype, L.kgdet_range_scan_blocks.argtypes = ctypes.c_int64, [ctypes.c_int64]
    L.kgdet_range_scan_chunk.restype, L.kgdet_range_scan_chunk.argtypes = ctypes.c_int32, []
    L.kgdet_range_scan_multi.restype = ctypes.c_int
    L.kgdet_range_scan_multi.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    return L


def _bits(x):
    return int(np.asarray(x, np.float32).view(np.uint32))


def _cases(big):
    """[(label, dict of envelope_refs.record's arguments)]; every generator seeded"""
    rng = np.random.default_rng(20260118)
    out = []
    for n in SMALL_COUNTS + [big]:
        out.append(('zeros n=%d' % n, dict(v=np.zeros(n, np.float32), hi1=HI1, hi2=HI2)))
        for what in (np.nan, np.inf, -np.inf):
            for where, pos in (('first', 0), ('middle', n // 2), ('last', n - 1)):
                v = (rng.standard_normal(n) * 100).astype(np.float32)
                v[pos] = what
                out.append(('%s %s n=%d' % (what, where, n), dict(v=v, hi1=HI1, hi2=HI2)))
        for label, edge in (('at hi1', HI1), ('above hi1', np.nextafter(HI1, np.float32(np.inf)))):
            v = rng.uniform(-1, 1, n).astype(np.float32)
            v[n - 1 - (n // 3)] = -edge if n % 2 else edge
            out.append(('%s n=%d' % (label, n), dict(v=v, hi1=HI1, hi2=HI2)))
        sub = rng.integers(1, 0x800000, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)
        out.append(('subnormals n=%d' % n, dict(v=sub.view(np.float32), hi1=HI1, hi2=HI2)))
    # weights with row scales: [O, inner], one row's running variance 1e-12 (s = 316), with and without gamma; an inner below 4
    # (a quad spans rows), a count that is no multiple of inner, and one row set beyond the capped grid
    for O, inner, count, with_gamma in ((16, 16 * 9, None, True), (13, 32, None, False), (22, 3, 65, True), (63, 1, None, False),
                                         (64, -(-big // 64), None, True)):
        count = O * inner if count is None else count
        v = rng.standard_normal(count).astype(np.float32)
        var = rng.uniform(0.5, 2.0, O).astype(np.float32)
        var[7] = 1e-12
        v[7 * inner] = 3.0                      # (row 7 leaves the envelope whatever the draw: 3 * 0.5 * 316 > 255.875)
        gamma = rng.uniform(0.5, 1.5, O).astype(np.float32) if with_gamma else None
        out.append(('scaled O=%d inner=%d n=%d' % (O, inner, count),
                    dict(v=v, hi1=HI1, hi2=HI2, inner=inner, var=var, eps=1e-5, gamma=gamma)))
    return out


@pytest.fixture(scope='module')
def scanned():
    L = _lib_scan()
    chunk, cap = L.kgdet_range_scan_chunk(), L.kgdet_range_scan_blocks(1 << 40)
    big = cap * chunk + 5                       # one element more than cap blocks cover in one trip: a second trip, and a tail
    assert L.kgdet_range_scan_blocks(big) == cap and L.kgdet_range_scan_blocks(chunk + 1) == 2 and L.kgdet_range_scan_blocks(1) == 1
    cases = _cases(big)
    n = len(cases)
    dev = torch.device('cuda')
    keep, rows, first, offsets = [], np.zeros((n, 8), np.int64), 0, []
    for i, (_, c) in enumerate(cases):
        count, off = c['v'].size, i % 4          # the base pointer 0 / 4 / 8 / 12 bytes behind a 16-byte boundary
        buf = torch.zeros(count + 4, dtype=torch.float32, device=dev)
        assert buf.data_ptr() % 16 == 0
        t = buf[off:off + count]
        t.copy_(torch.from_numpy(c['v'].view(np.int32)).view(torch.float32))     # (bit copy: NaNs and subnormals as they are)
        keep.append(buf)
        offsets.append((count, off))
        rows[i, 0], rows[i, 1] = t.data_ptr(), count
        if c.get('inner'):
            var = torch.from_numpy(c['var']).to(dev)
            gamma = torch.from_numpy(c['gamma']).to(dev) if c['gamma'] is not None else None
            keep += [var, gamma]
            rows[i, 2], rows[i, 3], rows[i, 4] = c['inner'], gamma.data_ptr() if gamma is not None else 0, var.data_ptr()
            rows[i, 5] = _bits(c['eps'])
        rows[i, 6] = _bits(c['hi1']) | (_bits(c['hi2']) << 32)
        rows[i, 7] = first
        first += L.kgdet_range_scan_blocks(count)
    table = torch.from_numpy(rows).to(dev)
    rec = torch.full((n + 2, 4), -1, dtype=torch.int32, device=dev)      # 0xFF everywhere; rows 0 and n + 1 are the canaries
    stream = _lib.raw_stream()
    got = []
    for _ in range(2):
        _lib.check(L.kgdet_range_scan_multi(table.data_ptr(), n, first, rec[1].data_ptr(), stream), 'range_scan_multi')
        got.append(rec.cpu().numpy().view(np.uint32))
    expect = ref.records([c for _, c in cases])
    return dict(cases=cases, first=got[0], second=got[1], expect=expect, offsets=offsets, big=big, cap=cap, chunk=chunk)


def test_every_count_meets_every_alignment(scanned):
    seen = set(scanned['offsets'])
    for n in SMALL_COUNTS + [scanned['big']]:
        assert {off for c, off in seen if c == n} == {0, 1, 2, 3}, n
    assert scanned['big'] > scanned['cap'] * scanned['chunk']


def test_canaries_and_relaunch(scanned):
    a, b = scanned['first'], scanned['second']
    assert (a[0] == 0xFFFFFFFF).all() and (a[-1] == 0xFFFFFFFF).all()
    assert np.array_equal(a, b)                 # overwritten by the second launch, not added to


def test_counts_equal_the_reference(scanned):
    got, expect = scanned['first'][1:-1], scanned['expect']
    for i, (label, _) in enumerate(scanned['cases']):
        assert (got[i, 1], got[i, 2], got[i, 3]) == (expect['nonfinite'][i], expect['over1'][i], expect['over2'][i]), label
    labels = [l for l, _ in scanned['cases']]
    for i, l in enumerate(labels):
        if l.startswith('at hi1'):
            assert got[i, 2] == 0 and got[i + 1, 2] == 1 and labels[i + 1].startswith('above hi1'), l
        if l.startswith(('nan', 'inf', '-inf')):
            assert got[i, 1] == 1, l
    assert expect['over1'].sum() > 0 and expect['over2'].sum() > 0


def test_max_is_bit_equal_without_a_row_scale(scanned):
    got, expect = scanned['first'][1:-1], scanned['expect']
    for i, (label, c) in enumerate(scanned['cases']):
        if not c.get('inner'):
            assert got[i, 0] == _bits(expect['max'][i]), label
        if label.startswith('subnormals'):
            assert 0 < got[i, 0] < 0x800000, label


def test_scaled_rows_within_four_ulps_and_clear_of_the_limits(scanned):
    got, expect = scanned['first'][1:-1], scanned['expect']
    n_scaled = 0
    for i, (label, c) in enumerate(scanned['cases']):
        if c.get('inner'):
            n_scaled += 1
            p = ref.products(c['v'], c['inner'], c['var'], c['eps'], c['gamma'])
            # the property of the INPUTS that makes exact counts a fair demand: no product within 2^-20 of a limit
            assert ref.margin(p, HI1) > 2.0 ** -20 and ref.margin(p, HI2) > 2.0 ** -20, label
            per_row = np.abs(p[:(p.size // c['inner']) * c['inner']].reshape(-1, c['inner'])).max(1)
            assert per_row[7] > HI1 and expect['over1'][i] > 0, label       # the tiny variance really leaves the envelope
            d = abs(int(got[i, 0]) - _bits(expect['max'][i]))
            print('%s: max %r against %r, %d ulps' % (label, got[i, 0:1].view(np.float32)[0], expect['max'][i], d))
            assert d <= 4, label
    assert n_scaled == 5
