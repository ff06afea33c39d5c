"""GPU parity of deformable convolutions with narrow, numerous weight groups -- what ``dcn['groups']`` of a ResNeXt block reaches
(32 groups of 4 ... 32 channels, stride 1 and 2) -- against the float64 oracle on the table of tests/dcn_group_cases.py, through
the public functions ``dcn.deform_conv`` / ``dcn.modulated_deform_conv``.  tests/test_dcn_group_cases.py holds the table, the
oracle and the routing facts on the CPU.

Tolerances are those of tests/test_gpu_dcn_edges.py for the same kernels: forward 2e-5 of the output scale ('split', 'exact'),
1e-2 ('bf16'); every gradient 5e-5.  EVERY element is compared.

Which kernel serves these shapes (csrc/dcn_api.hip; Cg = C / groups, Og = O / groups, HW = H * W of the input map):
  forward 'split' / 'bf16'   dg == 1: plane_ok, dcn_fwd_plane<2> / <1> with one sub-problem per weight group, at most kMaxFwdGroup
                             = 8 of them per launch (32 groups: four launches, the tap records rebuilt for each); Cg_pad = 16 and
                             Og_pad = 256, so with Cg = Og = 4 a stage carries 12 zero channels and a tile 252 zero rows.
                             HW > 1344: gather_ok, dcn_fwd_gather per weight group (C % 4 == 0; `8x1-1368px` has C = 8).
                             dg > 1 with deformable groups of fewer than 16 channels (`8x4-dg8`, `2x32-dg8`): neither plane_ok nor
                             gather_ok, the call runs on dcn_fwd_mfma whatever the precision asked for
  forward 'exact'            dcn_fwd_mfma + dcn_fwd_fixup per weight group
  backward_input, default    plane_bwd_offset_ok wants groups == 1 and dg == 1, or every deformable group inside one weight group
                             in whole 16-channel chunks: NO ResNeXt class (dg = 1, groups > 1) has that, so none of them runs
                             dcn_bwd_input_plane / dcn_bwd_offset_plane (plane_bwd_input_ok alone, which 8 runs pass and 9 / 32
                             fail, does not decide the route).  HW <= 1088 (plan_bwd_lds): dcn_bwd_build_index + per weight
                             group dcn_bwd_input_gather + dcn_bwd_input_fixup with n_cslices = 1 (a 32-channel slice of which
                             32 - Cg rows are dead), grad_offset summed over the groups * n_cslices slices by dcn_bwd_offset_fixup --
                             the same kernels as under 'exact'.  HW > 1088 (`8x4-1200px`, the three 1368-pixel cases): dcn_bwd_large
                             per channel run refuses Og % 16 != 0 and odd K * Cg before it launches anything, and
                             dcn._backward_input_padded runs the same kernels with every group zero-padded to 16 output channels
                             (and, Cg = 1, to two input channels, grad_input sliced back); grad_offset accumulates over the runs
  backward_input, 'exact'    the same two routes (the option only switches the plane kernels off)
  backward_weight, default   plane_ok / gather_ok: grad_weight_plane_grouped takes at most 8 channel runs per launch -- the 8-group
                             cases run dcn_bwd_weight_os<2> (HW > 1344: dcn_bwd_weight_gather<2>) --, 9 and 32 groups are refused
                             there and fall to one dcn_bwd_weight_mfma + dcn_bwd_weight_fixup per group, written into the packed
                             image at weight_images(s, d, g).fwd and unpacked by dcn_unpack_weight
  backward_weight, 'exact'   dcn_bwd_weight_mfma per group, every case
The second tier (deformable groups against narrow weight groups) either computes or raises NotImplementedError
(KGDET_E_UNSUPPORTED through _lib.check); `test_mixed_groups_compute_or_refuse` prints which.  Seen on an MI355X: `8x4-dg8` and
`8x8-dg2` compute everywhere; `2x32-dg8` refuses backward_weight (v1 and v2, both arithmetics: deformable groups of 8 channels have
no split-operand kernel and dcn_bwd_weight_mfma's channel tiles would straddle them) and computes the rest.

Worst error as a fraction of its bar on an MI355X (`EDGE-ERR GROUPS ...` lines): forward 0.24 'split', 0.11 'exact', 0.34 'bf16';
backward 0.21 over all gradients in the default and in the exact arithmetic (the same kernels serve backward_input in both), y
0.18 / 0.06; between NaN guards 0.15 / 0.11 / 0.34 forward and 0.14 over the gradients; second tier 0.26 at most.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import dcn_group_cases as G
from tests.test_gpu_dcn_edges import GRAD_TOL, PRECISIONS, _close, _poison_allocator

pytestmark = pytest.mark.gpu

GUARD = 64          # floats on both sides of a guarded operand: the payload keeps its 256-byte alignment
NAN = float('nan')
SENTINEL = 1.5      # prefill of grad_input in a refused call
VERSIONS = [(False, 'v1'), (True, 'v2')]


def _require_gpu():
    assert torch.cuda.is_available(), 'GPU tests need a GPU (no fallback)'


def _plain(a):
    return torch.from_numpy(np.array(a)).cuda()


def _guarded(a):
    """a contiguous view of `a`'s values between two guard regions of GUARD NaN floats"""
    a = np.array(a, np.float32)           # (a copy: the oracle's arrays are read-only)
    buf = torch.full((2 * GUARD + a.size,), NAN, dtype=torch.float32, device='cuda')
    view = buf[GUARD:GUARD + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * GUARD and view.data_ptr() % 256 == 0
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())
    return view


def _operands(r, v2, put=_plain, **replaced):
    """{x, off, w, go[, mask, bias]} on the device (`replaced`: other values for some of them); bias is never guarded"""
    names = ('x', 'off', 'w', 'go') + (('mask',) if v2 else ())
    ops = {n: put(replaced.get(n, r[n])) for n in names}
    if v2:
        ops['bias'] = _plain(r['bias'])
    return ops


def _forward(ops, case, v2, prec):
    from kgdet_amd import dcn
    N, C, H, W, O, k, s, p, d, g, dg = case
    with torch.no_grad(), dcn.forward_precision(prec):
        if v2:
            return dcn.modulated_deform_conv(ops['x'], ops['off'], ops['mask'], ops['w'], ops['bias'], s, p, d, g, dg)
        return dcn.deform_conv(ops['x'], ops['off'], ops['w'], s, p, d, g, dg)


def _autograd(ops, case, v2):
    """forward + ``y.backward(go)`` through the public functions: dict(y, grad_input, grad_offset, grad_weight[, grad_mask, grad_bias])"""
    from kgdet_amd import dcn
    N, C, H, W, O, k, s, p, d, g, dg = case
    tx, to, tw = (ops[n].requires_grad_() for n in ('x', 'off', 'w'))
    if v2:
        tm, tb = ops['mask'].requires_grad_(), ops['bias'].requires_grad_()
        y = dcn.modulated_deform_conv(tx, to, tm, tw, tb, s, p, d, g, dg)
    else:
        y = dcn.deform_conv(tx, to, tw, s, p, d, g, dg)
    y.backward(ops['go'])
    out = dict(y=y.detach(), grad_input=tx.grad, grad_offset=to.grad, grad_weight=tw.grad)
    if v2:
        out.update(grad_mask=tm.grad, grad_bias=tb.grad)
    return out


def _check(tag, got, r, v2):
    _close(tag + ' y', got['y'], r['y'], 2e-5)
    for name in G.grads(v2):
        _close('%s %s' % (tag, name), got[name], r[name], GRAD_TOL)


# ---------------------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize('case', G.RESNEXT_CASES, ids=G.case_id)
def test_forward_all_precisions(case):
    """v1, and v2 with mask and bias, under 'split', 'exact' and 'bf16': dcn_fwd_plane<2> / <1> in launches of at most eight weight
    groups (maps beyond 1344 pixels: dcn_fwd_gather per group) and dcn_fwd_mfma.  No refusal is allowed."""
    _require_gpu()
    for v2, ver in VERSIONS:
        r = G.reference(case, v2)
        for prec, tol in PRECISIONS:
            _poison_allocator()
            y = _forward(_operands(r, v2), case, v2, prec)
            _close('GROUPS forward %s %s %s' % (prec, G.case_id(case), ver), y, r['y'], tol)


# ------------------------------------------------------------------------------------------------------- 2. autograd backward
@pytest.mark.parametrize('mode', ['split', 'exact'], ids=['default', 'exact'])
@pytest.mark.parametrize('case', G.RESNEXT_CASES, ids=G.case_id)
def test_backward_every_gradient(case, mode):
    """``y.backward(go)``, v1 and v2, in the default arithmetic and under dcn.arithmetic('exact'), the allocator's free blocks
    NaN-filled before each call.  Maps of at most 1088 pixels: dcn_bwd_input_gather per weight group on a 32-channel slice with
    32 - Cg dead rows, grad_offset summed over the groups' slices; larger maps: dcn_backward_large.hip per channel run on the
    zero-padded groups of dcn._backward_input_padded.  grad_weight: dcn_bwd_weight_os<2> / dcn_bwd_weight_gather<2> up to 8 groups
    in the default arithmetic, one dcn_bwd_weight_mfma per group beyond that and under 'exact'.  No refusal is allowed."""
    _require_gpu()
    from kgdet_amd import dcn
    for v2, ver in VERSIONS:
        r = G.reference(case, v2)
        _poison_allocator()
        with dcn.arithmetic(mode):
            got = _autograd(_operands(r, v2), case, v2)
        _check('GROUPS backward %s %s %s' % ('default' if mode == 'split' else mode, G.case_id(case), ver), got, r, v2)


# ------------------------------------------------------------------------------------------ 3. operands at the end of memory
@pytest.mark.parametrize('case', G.GUARDED, ids=G.case_id)
def test_operands_between_nan_guards(case):
    """x, weight, offset, mask and grad_output each a contiguous view between 64 NaN floats on either side, default arithmetic:
    a 16-channel chunk of the last group that reads past C, a weight pack that reads past O * Cg * K or a grad_output row past
    O reaches a sum as NaN.  Every result finite and within the tolerances above."""
    _require_gpu()
    for v2, ver in VERSIONS:
        r = G.reference(case, v2)
        tag = 'GROUPS guarded %s %s' % (G.case_id(case), ver)
        for prec, tol in PRECISIONS:
            _poison_allocator()
            y = _forward(_operands(r, v2, _guarded), case, v2, prec)
            _close('%s forward %s' % (tag, prec), y, r['y'], tol)
        _poison_allocator()
        _check(tag + ' backward', _autograd(_operands(r, v2, _guarded), case, v2), r, v2)


# ------------------------------------------------------------------------------------------------ 4. groups do not see each other
def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize('case', G.ISOLATED, ids=G.case_id)
def test_groups_do_not_see_each_other(case):
    """x and weight of one weight group g0 (the first, a middle one, the last) replaced by other finite values: y and grad_weight of
    every other group, and grad_input of every other group's channels, keep their BITS; those of g0 change.  (grad_offset sums over
    all groups and is not compared.)"""
    _require_gpu()
    N, C, H, W, O, k, s, p, d, g, dg = case
    Cg, Og = C // g, O // g
    for v2, ver in VERSIONS:
        r = G.reference(case, v2)
        base = _autograd(_operands(r, v2), case, v2)
        for g0 in (0, g // 2, g - 1):
            rng = np.random.default_rng(100 + g0)
            x2, w2 = np.array(r['x']), np.array(r['w'])
            x2[:, g0 * Cg:(g0 + 1) * Cg] = rng.normal(size=(N, Cg, H, W)).astype(np.float32) * 3.0
            w2[g0 * Og:(g0 + 1) * Og] = rng.normal(size=(Og, Cg, k, k)).astype(np.float32) * 0.2
            got = _autograd(_operands(r, v2, x=x2, w=w2), case, v2)
            tag = '%s %s g0 = %d' % (G.case_id(case), ver, g0)
            for name, per, dim in (('y', Og, 1), ('grad_weight', Og, 0), ('grad_input', Cg, 1)):
                a, b = _bits(base[name]), _bits(got[name])
                assert bool(torch.isfinite(got[name]).all()), '%s: %s not finite' % (tag, name)
                own = torch.zeros(a.shape[dim], dtype=torch.bool, device=a.device)
                own[g0 * per:(g0 + 1) * per] = True
                sel = lambda t, m: t[:, m] if dim == 1 else t[m]
                assert torch.equal(sel(a, ~own), sel(b, ~own)), '%s: %s of another group changed' % (tag, name)
                assert not torch.equal(sel(a, own), sel(b, own)), '%s: %s of the group itself did not change' % (tag, name)


# ------------------------------------------------------------------------------------------------------------ 5. repeatability
@pytest.mark.parametrize('case', G.REPEATED, ids=G.case_id)
def test_backward_repeats_its_bits(case):
    """the kernels claim to have no atomics: forward and every gradient bit for bit the same on a second call, and on a third with
    an unrelated launch in between"""
    _require_gpu()
    for v2, ver in VERSIONS:
        r = G.reference(case, v2)
        a = _autograd(_operands(r, v2), case, v2)
        b = _autograd(_operands(r, v2), case, v2)
        other = torch.randn(1 << 20, device='cuda')          # an unrelated launch in between
        other.mul_(2.0)
        c = _autograd(_operands(r, v2), case, v2)
        for name in a:
            assert torch.equal(_bits(a[name]), _bits(b[name])), '%s %s %s differs between two runs' % (G.case_id(case), ver, name)
            assert torch.equal(_bits(a[name]), _bits(c[name])), '%s %s %s differs after an unrelated launch' % (G.case_id(case), ver, name)


# -------------------------------------------------------------------------------------------------------- 6. compute or refuse
def _refused_at_the_c_abi(entry, ops, case, v2, flags=0, exact=False):
    """the refused call once more at the C ABI -- the wrapper allocates its outputs itself and drops them when it raises --, every
    output prefilled by this test: NaN, and grad_input, which the kernels of some routes add to, with the finite value SENTINEL,
    so that a store of zeros and an added contribution both show.  KGDET_E_UNSUPPORTED again, and not one output element written"""
    from kgdet_amd import _lib, dcn
    L = _lib.lib()
    N, C, H, W, O, k, s, p, d, g, dg = case
    Ho, Wo = G.output_size(case)
    x, off, w, go = (ops[n].detach() for n in ('x', 'off', 'w', 'go'))
    mask, bias = (ops['mask'].detach(), ops['bias'].detach()) if v2 else (None, None)
    shape = dcn._shape(x, w, (s, s), (p, p), (d, d), g, dg)
    packed = dcn.pack_weight(w, shape)
    ws = dcn._workspace(x.device, L.kgdet_dcn_workspace_bytes(ctypes.byref(shape)))
    wsa = (_lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.current_stream())
    nan = lambda t: None if t is None else torch.full_like(t, NAN)
    L.kgdet_set_option(0, int(exact))
    try:
        if entry == 'forward':
            outs = dict(y=torch.full((N, O, Ho, Wo), NAN, device='cuda'))
            rc = L.kgdet_deform_conv_forward(ctypes.byref(shape), _lib.ptr(x), _lib.ptr(off), _lib.ptr(mask), _lib.ptr(packed),
                                             _lib.ptr(bias), _lib.ptr(outs['y']), ctypes.c_uint32(flags), *wsa)
        elif entry == 'backward_input':
            outs = dict(grad_input=torch.full_like(x, SENTINEL), grad_offset=nan(off), grad_mask=nan(mask))
            rc = L.kgdet_deform_conv_backward_input(ctypes.byref(shape), _lib.ptr(x), _lib.ptr(off), _lib.ptr(mask), _lib.ptr(packed),
                                                    _lib.ptr(go), _lib.ptr(outs['grad_input']), _lib.ptr(outs['grad_offset']),
                                                    _lib.ptr(outs['grad_mask']), *wsa)
        else:
            outs = dict(grad_weight=nan(w), grad_bias=nan(bias))
            rc = L.kgdet_deform_conv_backward_weight(ctypes.byref(shape), _lib.ptr(x), _lib.ptr(off), _lib.ptr(mask), _lib.ptr(go),
                                                     _lib.ptr(outs['grad_weight']), _lib.ptr(outs['grad_bias']), 0, *wsa)
    finally:
        L.kgdet_set_option(0, 0)
    torch.cuda.synchronize()
    assert rc == _lib.KGDET_E_UNSUPPORTED, '%s: refused through the wrapper, status %d at the C ABI' % (entry, rc)
    for name, t in outs.items():
        if t is not None:
            kept = bool((t == SENTINEL).all()) if name == 'grad_input' else bool(torch.isnan(t).all())
            assert kept, '%s refused, but %s was written' % (entry, name)


@pytest.mark.parametrize('case', G.MIXED_CASES, ids=G.case_id)
def test_mixed_groups_compute_or_refuse(case):
    """Deformable groups against narrow weight groups: each of forward (three precisions), backward-input and backward-weight
    (default and 'exact' arithmetic), v1 and v2, either meets its tolerance or raises NotImplementedError -- never another
    exception, never a finite wrong value --, and a refusal leaves every output of the call as this test prefilled it.  Prints the
    combinations that refused (`GROUPS-REFUSED`)."""
    _require_gpu()
    from kgdet_amd import dcn
    N, C, H, W, O, k, s, p, d, g, dg = case
    flags = {'split': 0, 'bf16': 2, 'exact': 4}
    refused = []
    for v2, ver in VERSIONS:
        r = G.reference(case, v2)
        tag = 'GROUPS mixed %s %s' % (G.case_id(case), ver)
        for prec, tol in PRECISIONS:
            ops = _operands(r, v2)
            _poison_allocator()
            try:
                y = _forward(ops, case, v2, prec)
            except NotImplementedError as e:
                refused.append(('forward', prec, ver, str(e)))
                _refused_at_the_c_abi('forward', ops, case, v2, flags=flags[prec])
                continue
            _close('%s forward %s' % (tag, prec), y, r['y'], tol)
        for mode in ('split', 'exact'):
            arith = 'default' if mode == 'split' else mode
            for entry, needs, names in (
                    ('backward_input', dict(input=True, offset=True, mask=v2, weight=False, bias=False),
                     ('grad_input', 'grad_offset') + (('grad_mask',) if v2 else ())),
                    ('backward_weight', dict(input=False, offset=False, mask=False, weight=True, bias=v2),
                     ('grad_weight',) + (('grad_bias',) if v2 else ()))):
                ops = _operands(r, v2)
                shape = dcn._shape(ops['x'], ops['w'], (s, s), (p, p), (d, d), g, dg)
                _poison_allocator()
                try:
                    with dcn.arithmetic(mode):
                        packed = dcn.pack_weight(ops['w'], shape)
                        res = dcn._backward(ops['x'], ops['off'], ops.get('mask'), ops['w'], ops.get('bias'), ops['go'], shape, packed, needs)
                except NotImplementedError as e:
                    refused.append((entry, arith, ver, str(e)))
                    _refused_at_the_c_abi(entry, ops, case, v2, exact=mode == 'exact')
                    continue
                got = dict(zip(('grad_input', 'grad_offset', 'grad_mask', 'grad_weight', 'grad_bias'), res))
                for name in names:
                    _close('%s %s %s %s' % (tag, entry, arith, name), got[name], r[name], GRAD_TOL)
    for entry, arith, ver, why in refused:
        print('GROUPS-REFUSED %s %s %s %s: %s' % (G.case_id(case), entry, arith, ver, why))
    print('GROUPS-REFUSALS %s: %d' % (G.case_id(case), len(refused)))
