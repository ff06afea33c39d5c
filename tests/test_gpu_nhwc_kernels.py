"""csrc/conv_nhwc.hip -- the bf16 channels-last 1x1 convolution with bias, residual and ReLU in its store, and the deferred input
epilogue -- through the C ABI against tests/nhwc_refs.py, all eight instantiations (ReLU x wave count x input epilogue), residual
given and NULL:

  exact tier   operands on a lattice on which every sum is exact: the output's 16-bit patterns equal the reference's, at the
               smallest shapes that reach each k-step count, tile edge, wave variant and trip count of the persistent loop;
  mixed tier   normal-distributed operands: every element inside [final(S - e), final(S + e)] around the float64 sum.

Every output sits in a guarded buffer pre-filled with bf16 NaN: each element of [M, N] is written, no word around it is.
"""
import numpy as np
import pytest
import torch

from tests import nhwc_refs as R
from tests.test_gpu_pointwise_kernels import E_SHAPE, Guarded, _L, _ptr, _st, c_i32, c_i64

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7fc0


def _bf16(a):
    """float32 array of bf16 values -> bf16 tensor on the device (an exact conversion)"""
    R.bf16_bits(a)
    return torch.from_numpy(np.array(a, np.float32)).cuda().to(torch.bfloat16)


def _f32(a):
    return torch.from_numpy(np.array(a, np.float32)).cuda()


def _nan_out(M, N):
    g = Guarded(max(M * N // 2, 4))
    g.view().view(torch.bfloat16).fill_(float('nan'))
    assert bool((g.view().view(torch.int16) == NAN_BITS).all())
    return g


def _launch(x, in_bias, w, bias, res, out, M, K, N, relu, in_epi):
    """in_epi: kgdet_conv1x1_nhwc_residual_in; otherwise the entry without an in_bias argument"""
    lib, L = _L()
    if in_epi:
        return L.kgdet_conv1x1_nhwc_residual_in(_ptr(x), _ptr(in_bias), _ptr(w), _ptr(bias), _ptr(res), out.ptr(), c_i64(M), c_i32(K),
                                                c_i32(N), c_i32(relu), _st())
    return L.kgdet_conv1x1_nhwc_residual(_ptr(x), _ptr(w), _ptr(bias), _ptr(res), out.ptr(), c_i64(M), c_i32(K), c_i32(N), c_i32(relu),
                                         _st())


def _out_bits(g, M, N):
    return g.view().view(torch.int16)[:M * N].cpu().numpy().view(np.uint16).reshape(M, N)


@pytest.mark.parametrize('combo', R.COMBOS, ids=R.combo_id)
@pytest.mark.parametrize('case', R.EXACT_CASES, ids=R.case_id)
def test_exact_tier_bit_for_bit(case, combo):
    K, N, M = case
    relu, in_epi, with_res = combo
    lib, L = _L()
    inp = R.exact_inputs(case)
    want = R.bf16_bits(R.exact_reference(case, combo)['out'])
    x = _bf16(R.activation(inp, in_epi))
    w, bias = _bf16(inp['w']), _f32(inp['bias'])
    in_bias = _f32(inp['in_bias']) if in_epi else None
    res = _bf16(inp['res']) if with_res else None
    out = _nan_out(M, N)
    lib.check(_launch(x, in_bias, w, bias, res, out, M, K, N, relu, in_epi), 'conv1x1_nhwc_residual')
    torch.cuda.synchronize()
    assert out.intact()
    got = _out_bits(out, M, N)
    wrong = got != want
    print('NHWC-EXACT %s %s: %d of %d elements differ' % (R.case_id(case), R.combo_id(combo), int(wrong.sum()), wrong.size))
    if wrong.any():
        m, n = np.argwhere(wrong)[0]
        raise AssertionError('%d of %d elements differ, first at row %d channel %d: %#06x, reference %#06x; rows %s ... channels %s' % (
            int(wrong.sum()), wrong.size, m, n, got[m, n], want[m, n], np.unique(np.argwhere(wrong)[:, 0])[:8],
            np.unique(np.argwhere(wrong)[:, 1])[:8]))


@pytest.mark.parametrize('K,combo', R.MIXED_CASES, ids=lambda v: R.combo_id(v) if isinstance(v, tuple) else 'K%d' % v)
def test_mixed_tier_inside_the_interval(K, combo):
    relu, in_epi, with_res = combo
    M, N = R.MIXED_M, R.MIXED_N
    lib, L = _L()
    inp, iv = R.mixed_inputs(K), R.mixed_interval(K, combo)
    out = _nan_out(M, N)
    lib.check(_launch(_bf16(inp['x']), _f32(inp['in_bias']) if in_epi else None, _bf16(inp['w']), _f32(inp['bias']),
                      _bf16(inp['res']) if with_res else None, out, M, K, N, relu, in_epi), 'conv1x1_nhwc_residual')
    torch.cuda.synchronize()
    assert out.intact()
    bits = _out_bits(out, M, N)
    got = (bits.astype(np.uint32) << 16).view(np.float32)
    assert np.isfinite(got).all()                                        # every element written
    lo_b, hi_b = R.bf16_bits(iv['lo']), R.bf16_bits(iv['hi'])
    pinned = lo_b == hi_b
    exact_wrong = pinned & (bits != lo_b)
    outside = ~pinned & ~((iv['lo'] <= got) & (got <= iv['hi']))
    at_end = ~pinned & ((bits == lo_b) | (bits == hi_b))
    print('NHWC-MIXED K%d %s: ambiguous %.4f; pinned wrong %d; outside %d; ambiguous elements on an end %d of %d' % (
        K, R.combo_id(combo), iv['ambiguous'], int(exact_wrong.sum()), int(outside.sum()), int(at_end.sum()), int((~pinned).sum())))
    assert not exact_wrong.any() and not outside.any()


@pytest.mark.parametrize('K,N', R.REFUSED)
def test_refused_sizes_leave_the_output_alone(K, N):
    lib, L = _L()
    M = 8
    x, w = torch.zeros(M * 528, dtype=torch.bfloat16, device='cuda'), torch.zeros(256 * 528, dtype=torch.bfloat16, device='cuda')
    bias, in_bias, res = torch.zeros(256, device='cuda'), torch.zeros(528, device='cuda'), torch.zeros(M * 256, dtype=torch.bfloat16, device='cuda')
    for in_epi in (0, 1):
        out = _nan_out(M, 256)
        assert _launch(x, in_bias, w, bias, res, out, M, K, N, 1, in_epi) == E_SHAPE
        torch.cuda.synchronize()
        assert out.intact() and bool((out.view().view(torch.int16) == NAN_BITS).all())


def test_no_rows_is_a_success_that_writes_nothing():
    lib, L = _L()
    for in_epi in (0, 1):
        out = _nan_out(8, 128)
        assert _launch(None, None, None, None, None, out, 0, 64, 128, 1, in_epi) == 0
        torch.cuda.synchronize()
        assert out.intact() and bool((out.view().view(torch.int16) == NAN_BITS).all())
