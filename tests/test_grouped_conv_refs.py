"""tests/grouped_conv_refs.py pinned on the CPU: the float64 operations written out over groups and taps equal
``F.conv2d(groups=)`` and its autograd in float64 to 1e-12, the lattice operands keep every sum exact, the case table holds what
the GPU tests rely on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import grouped_conv_refs as R

PIN = 1e-12


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


@pytest.mark.parametrize('name', R.NAMES)
def test_operations_equal_conv2d_and_its_autograd_in_float64(name):
    c = R.BY_NAME[name]
    op = R.mixed(name)
    x = torch.from_numpy(op.x).double().requires_grad_(True)
    w = torch.from_numpy(op.w).double().requires_grad_(True)
    y = F.conv2d(x, w, None, c.stride, 1, 1, c.groups)
    y.backward(torch.from_numpy(op.gy).double())
    (fwd, gi, gw), mag = R.results(name, 'mixed')
    assert fwd.shape == tuple(y.shape) == (c.B, c.groups * c.cpg, R.out_size(c.H, c.stride), R.out_size(c.W, c.stride))
    assert _rel(fwd, y.detach().numpy()) <= PIN
    assert _rel(gi, x.grad.numpy()) <= PIN
    assert _rel(gw, w.grad.numpy()) <= PIN
    # sum |a_i b_i| bounds every result
    for r, m in zip((fwd, gi, gw), mag):
        assert (np.abs(r) <= m * (1 + 1e-12)).all()


@pytest.mark.parametrize('name', R.NAMES)
def test_lattice_results_are_exact_floats_in_every_order(name):
    """sum |terms| of every result stays below 2^24 quanta, so every partial sum of every order is an exact float32"""
    c = R.BY_NAME[name]
    op = R.lattice(name)
    a = [np.abs(v).astype(np.float64) for v in (op.x, op.w, op.gy)]
    sums = (R.forward(a[0], a[1], c.stride) + np.abs(op.bias).astype(np.float64)[None, :, None, None],
            R.grad_input(a[2], a[1], c.H, c.W, c.stride), R.grad_weight(a[2], a[0], c.stride, c.cpg))
    for s, q in zip(sums, (2.0 ** (R.EA + R.EW), 2.0 ** (R.EG + R.EW), 2.0 ** (R.EG + R.EA))):
        assert s.max() < 2 ** 24 * q
        assert (np.round(s / q) == s / q).all()
    (fwd, gi, gw), _ = R.results(name, 'lattice')
    for r in (fwd, gi, gw):
        assert (r.astype(np.float32).astype(np.float64) == r).all()


def test_case_table_covers_every_class_map_group_count_and_batch():
    seen = {(c.cpg, c.stride) for c in R.CASES}
    assert seen == {(cpg, s) for cpg in R.CPGS for s in (1, 2)}
    assert {c.groups for c in R.CASES} == {1, 3, 32} and {c.B for c in R.CASES} == {1, 3}
    assert all(c.cpg in (4, 8) for c in R.CASES if c.groups == 32)
    assert all(c.groups == 3 for c in R.CASES if (c.H, c.W) in R.LARGE_MAPS)
    for cpg in R.CPGS:
        for s in (1, 2):
            maps = {(c.H, c.W) for c in R.CASES if (c.cpg, c.stride) == (cpg, s)}
            assert maps == set(R.SMALL_MAPS) | set(R.LARGE_MAPS)
    assert len(set(R.NAMES)) == len(R.NAMES)
    # the weight gradient's second pixel chunk and the second workgroup of a plane are reached
    assert any(c.B * R.out_size(c.H, c.stride) * R.out_size(c.W, c.stride) >= 16384 for c in R.CASES)
    assert any(R.out_size(c.H, c.stride) * -(-R.out_size(c.W, c.stride) // 4) > 256 for c in R.CASES)


def test_gamma_is_the_standard_bound():
    assert R.gamma(36) == pytest.approx(36 * 2.0 ** -24, rel=1e-5)
    assert R.gamma(1) > R.U
