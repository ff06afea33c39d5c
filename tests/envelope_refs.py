"""numpy restatement of the record of kgdet_range_scan_multi (include/kgdet_hip.h, kgdet_amd/csrc/range_scan.hip): float32
products, one rounding per operation -- s = gamma / sqrt(var + eps) is three float32 operations (add, square root, division; numpy's
are correctly rounded), the product v * s a fourth.  Shared by tests/test_envelope_refs.py (host logic against a fake scan) and the
GPU tests of the kernel and of the guard."""
import numpy as np

RECORD = np.dtype([('max', '<f4'), ('nonfinite', '<u4'), ('over1', '<u4'), ('over2', '<u4')])
F32 = np.float32


def row_scale(var, eps, gamma=None):
    with np.errstate(all='ignore'):
        root = np.sqrt((np.asarray(var, F32) + F32(eps)).astype(F32)).astype(F32)
        num = np.asarray(gamma, F32) if gamma is not None else np.ones_like(root)
        return (num / root).astype(F32)


def products(v, inner=0, var=None, eps=0.0, gamma=None):
    """the float32 products v[i] * s[i // inner] (the values themselves without a row scale), flat"""
    v = np.ascontiguousarray(v, dtype=F32).reshape(-1)
    if not inner or var is None:
        return v
    s = row_scale(var, eps, gamma)
    rows = np.arange(v.size, dtype=np.int64) // int(inner)
    with np.errstate(all='ignore'):
        return (v * s[rows]).astype(F32)


def record(v, hi1, hi2, inner=0, var=None, eps=0.0, gamma=None):
    """(max |p| over the finite products as float32 -- 0 when there is none --, non-finite count, count of |p| > hi1, of |p| > hi2);
    an infinite product counts beyond both limits, a NaN beyond neither"""
    a = np.abs(products(v, inner, var, eps, gamma))
    fin = np.isfinite(a)
    with np.errstate(invalid='ignore'):
        return (F32(a[fin].max()) if fin.any() else F32(0), int((~fin).sum()), int((a > F32(hi1)).sum()), int((a > F32(hi2)).sum()))


def records(rows):
    """rows: dicts of `record`'s arguments -> structured array like the kernel's read-back"""
    out = np.zeros(len(rows), dtype=RECORD)
    for i, r in enumerate(rows):
        out[i] = record(**r)
    return out


def margin(p, hi):
    """the smallest relative distance of a finite |p| from the limit ``hi`` (tests keep it above 2^-20 for generated inputs, so that
    no count can hinge on the last bits of a product)"""
    a = np.abs(np.asarray(p, np.float64))
    a = a[np.isfinite(a)]
    return float(np.abs(a / float(hi) - 1.0).min()) if a.size else float('inf')


def ulps(a, b):
    """distance of two non-negative finite float32 values in units of the last place"""
    return abs(int(np.asarray(a, F32).view(np.uint32)) - int(np.asarray(b, F32).view(np.uint32)))
