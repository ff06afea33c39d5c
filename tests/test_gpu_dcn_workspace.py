"""The deformable-convolution entry points of csrc/dcn_api.hip held to their workspace contract, through the C ABI.

Every other DCN test goes through kgdet_amd/dcn.py, whose one workspace per stream only grows and is never cleared: a size query
that is too small, a route that depends on spare room and a read of bytes the call did not write are all invisible there.  Here
the workspace, the packed weight and every output are exactly as large as the queries say, 256-byte aligned, between two guard
regions of 1 MiB each; outputs are prefilled with NaN (grad_input of kgdet_deform_conv_backward_input with the zeros its contract
asks for, grad_weight / grad_bias of an accumulating call with known values).  Per (entry point, case), `_contract`:

  a  size = the query (kgdet_dcn_workspace_bytes / kgdet_dcn_group_workspace_bytes), all-zero bytes: KGDET_OK -- KGDET_E_UNSUPPORTED
     exactly where include/kgdet_hip.h says the shape is declined --, every guard intact, the inputs unchanged, the result within the
     tolerances of tests/test_gpu_dcn_edges.py of the float64 oracle (forward 2e-5 of the output scale, bf16 forward 1e-2, every
     gradient 5e-5)
  b  size = 2 x the query (what the Python wrapper's grown buffer looks like): the bits of (a)
  c  the leftover of the same call on another draw (seed + 1) and of another entry point on the same shape: the bits of (a).
     Leftovers of the same shape on purpose: every stale index is in range, a stale read is a wrong number, never a wild address
  d  size = query - 256, size = what the entry point itself asks for when it refuses (NULL, 0) ("need N bytes"), and (NULL, 0):
     KGDET_E_WORKSPACE / KGDET_E_UNSUPPORTED with kgdet_last_error() set and every output still holding its prefill, or KGDET_OK with
     the bits of (a); (NULL, 0) must refuse

Which kernel serves which case (csrc/dcn_api.hip; HW = H * W, kPlaneMaxHW = 1344; E.SMALL_CASES are the maps up to 1344 pixels,
E.LARGE_CASES the two 38 x 36 ones):
  kgdet_dcn_pack_weight / _multi / _images    dcn_pack_weight_all / dcn_pack_weight_all_multi (groups == 1), all four images;
                                              kgdet_dcn_unpack_weight_grad (dcn_unpack_weight) returns the weight from the fp32 image
  kgdet_deform_conv_forward 0 / BF16          small: dcn_build_taps + dcn_fwd_plane<2> / <1> (+ blocked input copy behind the records),
                                              large: dcn_to_pixel_major + dcn_fwd_gather<2> / <1>; fix-up dcn_fwd_fixup[_static]
  kgdet_deform_conv_forward EXACT_FP32        dcn_fwd_mfma + dcn_fwd_fixup (slabs only)
  kgdet_deform_conv_grad_input                small: dcn_build_inverse_taps, dcn_inv_medium_sums / dcn_inv_overflow_sums,
                                              dcn_bwd_input_plane<2>; large: declined (KGDET_E_UNSUPPORTED)
  kgdet_deform_conv_grad_offset               small: dcn_build_grad_taps + dcn_bwd_offset_plane<2>; 2x32x6x7x32: dcn_bwd_offset_pair (O % 32
                                              == 0 and the static schedule; blocked input copy behind the records when there is room,
                                              plane switches through registers when not); large: declined
  kgdet_deform_conv_backward_input            small, default: the two above, v2: dcn_bwd_offset_plane_masked; small, exact option:
                                              dcn_bwd_build_index + dcn_bwd_input_gather; large: dcn_backward_large.hip per channel run
  kgdet_deform_conv_backward_weight           accumulate 0: small dcn_bwd_weight_os<2> (stream-K option: dcn_bwd_weight_plane<2> + fix-up),
                                              large dcn_bwd_weight_gather<2>; accumulate 1: dcn_bwd_weight_mfma + dcn_bwd_weight_fixup +
                                              kgdet_dcn_unpack_weight_grad; grad_bias: dcn_bias_grad
  grouped entry points (head stage)           dcn_fwd_plane<2>; dcn_bwd_input_prepare, dcn_hot_gemm, dcn_inv_medium_sums,
                                              dcn_bwd_input_plane<2>, dcn_bwd_offset_plane<2> (O = 16); dcn_bwd_weight_os<2> / stream-K

No two runs of one call may differ in a bit: the schedules (grids, ranges, parts) are functions of the shapes and the compute-unit
count alone, and the one thing spare room changes -- the blocked input copy of the tap-pair grad_offset kernel against the hand-over
through registers -- moves the same float32 planes into LDS by another road and leaves every sum in its order.  Each case prints
its query and which of the two hand-overs ran at every size (`WS-QUERY`, `WS-HANDOVER` lines; kgdet_debug_dcn_offset_handover
reports it).  The tap-pair kernel needs the static schedule of plan_static_ranges, which none of the 16-channel shapes gets (their
two pixel tiles share one workgroup): 2x32x6x7x32, the first shape with 32 channels instead of 16, is the smallest that does, and
there both hand-overs are REQUIRED to have run -- the blocked copy at the query, registers at the entry point's own minimum.  The
head stage's grouped grad_offset (six 16-channel problems) stays on dcn_bwd_offset_plane<2> at every size.
"""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

import oracle
from tests import dcn_edge_cases as E

pytestmark = pytest.mark.gpu

SEED = 7
GUARD = 1 << 20
CANARY = 0xA5
NAN = float('nan')
FWD_TOL = {0: 2e-5, 2: 1e-2, 4: 2e-5}      # by forward flag: split, KGDET_DCN_BF16, KGDET_DCN_EXACT_FP32
GRAD_TOL = 5e-5
OK, E_WORKSPACE, E_UNSUPPORTED = 0, 2, 4
REFUSALS = (E_WORKSPACE, E_UNSUPPORTED)
OPT_EXACT_BACKWARD, OPT_WGRAD_STREAMK = 0, 2


def _L():
    from kgdet_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need a GPU (no fallback)'
    return _lib.lib()


def _st():
    from kgdet_amd import _lib
    return ctypes.c_void_p(_lib.raw_stream())


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Bytes(object):
    """``size`` bytes, 256-byte aligned, between two regions of at least GUARD bytes of CANARY"""

    def __init__(self, size, fill=None):
        self.size = int(size)
        self.raw = torch.full((GUARD + self.size + GUARD + 256,), CANARY, dtype=torch.uint8, device='cuda')
        self.lead = GUARD + (-(self.raw.data_ptr() + GUARD)) % 256
        if fill is not None:
            self.f32().copy_(fill.reshape(-1)) if torch.is_tensor(fill) else self.f32().fill_(fill)

    def payload(self):
        return self.raw[self.lead:self.lead + self.size]

    def f32(self):
        return self.payload().view(torch.float32)

    def ptr(self):
        return ctypes.c_void_p(self.raw.data_ptr() + self.lead)

    def intact(self):
        front, back = self.raw[:self.lead], self.raw[self.lead + self.size:]
        return bool(((front == CANARY).all() & (back == CANARY).all()).item())


def _cuda(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # (a copy: the oracle's arrays are read-only)


def _shape(case, o_base=0, o_total=0):
    from kgdet_amd import _lib
    N, C, H, W, O, k, s, p, d, g, dg = case
    return _lib.DcnShape(N, C, H, W, O, k, k, s, s, p, p, d, d, g, dg, o_base, o_total)


def _set_option(option, value):
    from kgdet_amd import _lib
    _lib.check(_L().kgdet_set_option(option, value), 'kgdet_set_option')


class Problem(object):
    """one convolution's operands on the device (x, off, w, go, mask, bias: numpy arrays; go spans the whole output buffer of
    the shape's channel window) and its packed weight, packed into a NaN-prefilled guarded buffer of exactly the queried size"""

    def __init__(self, case, t, o_base=0, o_total=0):
        L = _L()
        self.case, self.shape = case, _shape(case, o_base, o_total)
        self.window = (o_base, o_base + case[4], o_total or case[4])
        self.t = {k: _cuda(v) for k, v in t.items()}
        self.keep = {k: v.clone() for k, v in self.t.items() if v is not None}
        nbytes = L.kgdet_dcn_packed_weight_bytes(ctypes.byref(self.shape))
        assert nbytes > 0 and nbytes % 4 == 0
        self.packed = Bytes(nbytes, NAN)
        assert L.kgdet_dcn_pack_weight(ctypes.byref(self.shape), _p(self.t['w']), self.packed.ptr(), _st()) == OK
        torch.cuda.synchronize()
        assert self.packed.intact(), 'kgdet_dcn_pack_weight wrote outside kgdet_dcn_packed_weight_bytes'
        self.packed_keep = self.packed.payload().clone()

    def untouched(self):
        return (all(torch.equal(v, self.t[k]) for k, v in self.keep.items()) and self.packed.intact() and
                torch.equal(self.packed.payload(), self.packed_keep))


class Call(object):
    """one entry point on one problem (or group): ``outs`` {name: (shape, prefill)}, ``launch(L, ws_ptr, ws_bytes, {name: ptr})``,
    ``refs`` {name: (float64 oracle, tolerance)} (the output's channel window where the problem has one), ``option`` a
    kgdet_set_option switch held during the launch, ``declined``: include/kgdet_hip.h promises KGDET_E_UNSUPPORTED for the shape
    (None: either), ``offset``: the call launches a grad_offset kernel (its hand-over variant is reported)"""

    def __init__(self, name, problems, outs, launch, refs=None, option=None, declined=False, offset=False, windows=None):
        self.name, self.problems, self.outs, self.launch, self.refs = name, problems, outs, launch, refs or {}
        self.option, self.declined, self.offset, self.windows = option, declined, offset, windows or {}

    def fresh_outs(self):
        return {k: Bytes(4 * int(np.prod(shape)), fill) for k, (shape, fill) in self.outs.items()}

    def run(self, ws, size):
        """one launch with workspace_bytes = `size` = ws.size (ws None: NULL, 0) -> (status, fresh outputs, grad_offset hand-over)"""
        L = _L()
        assert ws is None or ws.size == size
        outs = self.fresh_outs()
        if self.option is not None:
            _set_option(self.option, 1)
        try:
            rc = self.launch(L, ws.ptr() if ws is not None else None, ctypes.c_size_t(size), {k: b.ptr() for k, b in outs.items()})
        finally:
            if self.option is not None:
                _set_option(self.option, 0)
        torch.cuda.synchronize()
        what = '%s at %d bytes' % (self.name, size)
        assert ws is None or ws.intact(), what + ': write outside the workspace'
        for k, b in outs.items():
            assert b.intact(), '%s: write outside %s' % (what, k)
        for P in self.problems:
            assert P.untouched(), what + ': an input or the packed weight changed'
        return rc, outs, (L.kgdet_debug_dcn_offset_handover() if self.offset and rc == OK else None)

    def holds_prefill(self, outs):
        fresh = self.fresh_outs()
        return all(torch.equal(outs[k].payload(), fresh[k].payload()) for k in outs)


def _same_bits(a, b):
    return [k for k in a if not torch.equal(a[k].payload(), b[k].payload())]


def _close(what, actual, desired, tol):
    """every element within `tol` of the oracle's scale; prints the figure before it asserts (tests/test_gpu_dcn_edges.py)"""
    actual = actual.detach().cpu().numpy()
    assert actual.shape == desired.shape, (what, actual.shape, desired.shape)
    assert np.isfinite(actual).all(), '%s: non-finite values' % what
    scale = max(float(np.abs(desired).max()), 1e-6)
    err = float(np.abs(actual.astype(np.float64) - desired).max()) / scale
    print('WS-ERR %s err %.3e tol %.1e frac %.3f' % (what, err, tol, err / tol))
    assert err < tol, '%s: max error %.3e of the scale (tol %.1e)' % (what, err, tol)


HANDOVER = {None: '-', -1: 'no tap-pair kernel'}


def _handover(h):
    return HANDOVER.get(h, 'through registers' if h == 0 else 'blocked copy x %s' % h)


def _refused(call, rc, outs, what):
    assert rc in REFUSALS, '%s: status %d' % (what, rc)
    assert _L().kgdet_last_error(), what + ': refused without a message'
    assert call.holds_prefill(outs), what + ': refused, but an output was written'


def _contract(call, twin, other, sizes, tag):
    """(a) - (d) of the module docstring for `call`; `twin`: the same call on another draw, `other`: another entry point on the
    same shape; `sizes`: {'query', 'double', 'short': Bytes}"""
    L = _L()
    q = sizes['query']
    what = '%s %s' % (tag, call.name)
    # ---- a
    q.payload().zero_()
    rc, base, h_q = call.run(q, q.size)
    if call.declined or (call.declined is None and rc == E_UNSUPPORTED):
        # a shape the header says is declined (declined None: may be, "before anything is launched for that quantity"): the same
        # answer whatever the room, and nothing written where the header promises so
        assert rc == E_UNSUPPORTED, '%s: status %d, the header promises KGDET_E_UNSUPPORTED' % (what, rc)
        assert L.kgdet_last_error(), what + ': declined without a message'
        assert call.declined is None or call.holds_prefill(base), what + ': declined, but an output was written'
        print('WS-DECLINED %s: %s' % (what, L.kgdet_last_error().decode()))
        for key in ('double', 'short'):
            sizes[key].payload().zero_()
            rc2, outs, _ = call.run(sizes[key], sizes[key].size)
            assert rc2 == E_UNSUPPORTED or (key == 'short' and rc2 == E_WORKSPACE), '%s: declined at the query, status %d at %s' % (what, rc2, key)
            assert not _same_bits(base, outs) or (key == 'short' and call.holds_prefill(outs)), what + ': other bits at ' + key
        return
    assert rc == OK, '%s: status %d (%s)' % (what, rc, L.kgdet_last_error())
    for k, (ref, tol) in call.refs.items():
        got = base[k].f32().reshape(call.outs[k][0])
        if k in call.windows:
            lo, hi, total = call.windows[k]
            rest = torch.cat([got[:, :lo], got[:, hi:]], 1)
            assert bool(torch.isnan(rest).all()), '%s: %s written outside its channel window' % (what, k)
            got = got[:, lo:hi]
        _close('%s %s' % (what, k), got, ref, tol)
    # ---- b
    d = sizes['double']
    d.payload().zero_()
    rc, outs, h_d = call.run(d, d.size)
    assert rc == OK and not _same_bits(base, outs), '%s: 2 x query: status %d, differing %r' % (what, rc, _same_bits(base, outs))
    # ---- c
    for leftover in (twin, other):
        rc0, _, _ = leftover.run(q, q.size)
        assert rc0 == OK or (rc0 == E_UNSUPPORTED and leftover.declined is not False), (what, leftover.name, rc0)
        rc, outs, _ = call.run(q, q.size)
        assert rc == OK and not _same_bits(base, outs), '%s on the leftover of %s (%s): status %d, differing %r' % (
            what, leftover.name, 'another draw' if leftover is twin else 'another entry point', rc, _same_bits(base, outs))
    # ---- d
    rc, outs, _ = call.run(None, 0)
    _refused(call, rc, outs, what + ' (NULL, 0)')
    need = re.search(r'need (\d+) bytes', L.kgdet_last_error().decode())
    small = [sizes['short']]
    if need and int(need.group(1)) <= q.size:       # the entry point's own figure: exactly that much, guards right behind it
        small.append(Bytes(int(need.group(1))))
    h_s = []
    for ws in small:
        ws.payload().zero_()
        rc, outs, h = call.run(ws, ws.size)
        if rc == OK:
            assert not _same_bits(base, outs), '%s at %d bytes: KGDET_OK with other bits in %r' % (what, ws.size, _same_bits(base, outs))
        else:
            _refused(call, rc, outs, '%s at %d bytes' % (what, ws.size))
        h_s.append((ws.size, rc, h))
    if call.offset:
        print('WS-HANDOVER %s: query %d: %s; 2 x query: %s; %s' % (what, q.size, _handover(h_q), _handover(h_d), '; '.join(
            '%d bytes: %s' % (n, _handover(h) if rc == OK else 'refused') for n, rc, h in h_s)))
    return [h_q, h_d] + [h for n, rc, h in h_s if rc == OK]


# ------------------------------------------------------------------------------------------------- the single entry points
def _numel(*dims):
    return tuple(int(v) for v in dims)


def _single_calls(P, R1=None, R2=None, v2=True, tag=''):
    """every variant of the single-call entry points on problem P; R1 / R2: the v1 / v2 oracle results (None: no comparison)"""
    case, s, t, pk = P.case, ctypes.byref(P.shape), P.t, P.packed
    N, C, H, W, O, k, st_, pd, dl, g, dg = case
    Ho, Wo = E.output_size(case)
    lo, hi, total = P.window
    y_shape, plane = (N, total, Ho, Wo), H * W <= 1344 and Ho * Wo <= 1344
    x, off, w, go = t['x'], t['off'], t['w'], t['go']
    win = {'y': P.window} if total != O else {}
    ref = lambda R, name, tol: {} if R is None else {name: (R[name], tol)}
    calls = []

    def add(name, outs, launch, refs, **kw):
        calls.append(Call(tag + name, [P], outs, launch, refs, **kw))
    for ver, R in (('v1', R1), ('v2', R2)) if v2 else (('v1', R1),):
        mask, bias = (t['mask'], t['bias']) if ver == 'v2' else (None, None)
        for fname, flags in (('split', 0), ('bf16', 2), ('exact', 4)):
            add('forward %s %s' % (ver, fname), {'y': (y_shape, NAN)},
                lambda L, wp, wb, o, mask=mask, bias=bias, flags=flags: L.kgdet_deform_conv_forward(
                    s, _p(x), _p(off), _p(mask), pk.ptr(), _p(bias), o['y'], ctypes.c_uint32(flags), wp, wb, _st()),
                ref(R, 'y', FWD_TOL[flags]), windows=win)
        add('grad_input %s' % ('plain' if mask is None else 'masked'), {'grad_input': (x.shape, NAN)},
            lambda L, wp, wb, o, mask=mask: L.kgdet_deform_conv_grad_input(
                s, _p(off), _p(mask), pk.ptr(), _p(go), o['grad_input'], ctypes.c_uint32(0), wp, wb, _st()),
            ref(R, 'grad_input', GRAD_TOL), declined=not plane)
        outs = {'grad_input': (x.shape, 0.0), 'grad_offset': (off.shape, NAN)}
        refs = dict(ref(R, 'grad_input', GRAD_TOL), **ref(R, 'grad_offset', GRAD_TOL))
        if mask is not None:
            outs['grad_mask'] = (mask.shape, NAN)
            refs.update(ref(R, 'grad_mask', GRAD_TOL))
        for mode, option in (('default', None), ('exact', OPT_EXACT_BACKWARD)):
            add('backward_input %s %s' % (ver, mode), outs,
                lambda L, wp, wb, o, mask=mask: L.kgdet_deform_conv_backward_input(
                    s, _p(x), _p(off), _p(mask), pk.ptr(), _p(go), o['grad_input'], o['grad_offset'], o.get('grad_mask'), wp, wb, _st()),
                refs, option=option, offset=option is None)
        rng = np.random.default_rng(SEED + 300)
        for acc in (0, 1):
            # (an accumulating call adds to known values of the gradient's own magnitude, 0.05: the float32 addition rounds by
            # 2^-24 of the sum, three orders below the gradient tolerance)
            fill_w = _cuda((rng.normal(size=tuple(w.shape)) * 0.05).astype(np.float32)) if acc else NAN
            fill_b = _cuda((rng.normal(size=(O,)) * 0.05).astype(np.float32)) if acc else NAN
            outs = {'grad_weight': (w.shape, fill_w)}
            refs = {} if R is None else {'grad_weight': (R['grad_weight'] + (fill_w.cpu().numpy() if acc else 0.0), GRAD_TOL)}
            if bias is not None:
                outs['grad_bias'] = ((O,), fill_b)
                if R is not None:
                    refs['grad_bias'] = (R['grad_bias'] + (fill_b.cpu().numpy() if acc else 0.0), GRAD_TOL)
            for sched, option in (('', None), (' stream-K', OPT_WGRAD_STREAMK)) if not acc and mask is None else (('', None),):
                add('backward_weight %s accumulate %d%s' % (ver, acc, sched), outs,
                    lambda L, wp, wb, o, mask=mask, acc=acc: L.kgdet_deform_conv_backward_weight(
                        s, _p(x), _p(off), _p(mask), _p(go), o['grad_weight'], o.get('grad_bias'), ctypes.c_int(acc), wp, wb, _st()),
                    refs, option=option)
    add('grad_offset', {'grad_offset': (off.shape, NAN)},
        lambda L, wp, wb, o: L.kgdet_deform_conv_grad_offset(
            s, _p(x), _p(off), pk.ptr(), _p(go), o['grad_offset'], ctypes.c_uint32(0), wp, wb, _st()),
        ref(R1, 'grad_offset', GRAD_TOL), declined=H * W > 1344, offset=True)
    return calls


def _other_of(name, by_name, tag=''):
    """the entry point whose leftover `name` runs on: another one that writes tables where this one puts its own"""
    key = name[len(tag):]
    if key.startswith('forward'):
        pick = 'backward_weight v1 accumulate 0'       # grad_weight's records and grad_out images where the forward puts its records
    elif key.startswith('grad_input'):
        pick = 'grad_offset' if not by_name[tag + 'grad_offset'].declined else 'backward_weight v1 accumulate 0'
    elif key.startswith('grad_offset'):
        pick = 'grad_input plain'
    elif key.startswith('backward_input'):
        pick = 'backward_weight v1 accumulate 0'
    else:
        pick = 'backward_input v1 default'
    return by_name[tag + pick]


@functools.lru_cache(maxsize=None)
def _ref(case, v2):
    """float64 oracle of (case, edge offsets, v1 / v2): computed once, shared, read-only"""
    return E.reference(case, 'edge', v2, SEED)


def _draw(case, seed):
    """the operands of E.reference(case, 'edge', *, seed) without the oracle"""
    x, w, go, bias = E.tensors(case, seed)
    return dict(x=x, off=E.edge_offsets(case, seed + 100), w=w, go=go, mask=E.edge_mask(case, seed + 200), bias=bias)


def _sizes(query):
    assert query > 256
    return {'query': Bytes(query), 'double': Bytes(2 * query), 'short': Bytes(query - 256)}


PAIR_CASE = (2, 32, 6, 7, 32, 3, 1, 1, 1, 1, 1)      # the one shape of E.CASES whose grad_offset runs on the tap-pair kernel
assert PAIR_CASE in E.SMALL_CASES
FAMILIES = ('forward', 'grad_', 'backward_input', 'backward_weight')


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('case', E.SMALL_CASES + E.LARGE_CASES, ids=E.case_id)
def test_single_entry_points(case, family):
    """kgdet_deform_conv_forward (v1, v2; flags 0, BF16, EXACT_FP32), _grad_input (plain, masked), _grad_offset, _backward_input (v1,
    v2; default and the exact option) and _backward_weight (accumulate 0 / 1, without / with bias, the stream-K option) on
    kgdet_dcn_workspace_bytes: (a) - (d) of the module docstring."""
    L = _L()
    r1, r2 = _ref(case, False), _ref(case, True)
    assert all(np.array_equal(r1[k], r2[k]) for k in ('x', 'off', 'w', 'go'))
    P = Problem(case, {k: r2[k] for k in ('x', 'off', 'w', 'go', 'mask', 'bias')})
    P1 = Problem(case, _draw(case, SEED + 1))
    query = L.kgdet_dcn_workspace_bytes(ctypes.byref(P.shape))
    print('WS-QUERY %s: kgdet_dcn_workspace_bytes %d, kgdet_dcn_packed_weight_bytes %d' % (E.case_id(case), query, P.packed.size))
    calls, twins = _single_calls(P, r1, r2), {c.name: c for c in _single_calls(P1)}
    by_name = {c.name: c for c in calls}
    sizes = _sizes(query)
    for call in calls:
        if call.name.startswith(family):
            ran = _contract(call, twins[call.name], _other_of(call.name, by_name), sizes, E.case_id(case))
            if case == PAIR_CASE and call.name in ('grad_offset', 'backward_input v1 default'):
                # both hand-overs of the tap-pair kernel ran, and returned the same bits: the blocked copy where there is room
                # (the query, 2 x the query), registers where the workspace ends behind the records
                # (kgdet_deform_conv_grad_offset's own minimum; kgdet_deform_conv_backward_input asks for its grad_input tables too)
                assert ran[0] == ran[1] == 1 and (0 in ran[2:] or call.name != 'grad_offset'), \
                    '%s: the hand-overs that ran: %r' % (call.name, ran)


# ------------------------------------------------------------------------------------------------------------- the packers
@pytest.mark.parametrize('case', E.SMALL_CASES + E.LARGE_CASES, ids=E.case_id)
def test_packers(case):
    """kgdet_dcn_pack_weight, _multi and _images (fp32 images, then split images: all four) write the same bits into NaN-prefilled
    buffers of kgdet_dcn_packed_weight_bytes -- every byte a kernel reads is written by the packer, or it would show as NaN in the
    results of the tests above, which all read such a buffer --, and kgdet_dcn_unpack_weight_grad returns the weight itself from
    the fp32 image, accumulate 0 and 1."""
    L = _L()
    P = Problem(case, _draw(case, SEED))
    s, w = P.shape, P.t['w']
    arr = lambda v: (ctypes.c_void_p * 1)(v)
    shapes = (ctypes.POINTER(type(s)) * 1)(ctypes.pointer(s))
    multi, images = Bytes(P.packed.size, NAN), Bytes(P.packed.size, NAN)
    assert L.kgdet_dcn_pack_weight_multi(1, shapes, arr(w.data_ptr()), arr(multi.ptr().value), _st()) == OK
    for bits in (1, 2):
        assert L.kgdet_dcn_pack_weight_images(1, shapes, arr(w.data_ptr()), arr(images.ptr().value), ctypes.c_uint32(bits), _st()) == OK
    torch.cuda.synchronize()
    assert multi.intact() and images.intact() and P.untouched()
    assert torch.equal(multi.payload(), P.packed.payload()), 'kgdet_dcn_pack_weight_multi: other bits than kgdet_dcn_pack_weight'
    assert torch.equal(images.payload(), P.packed.payload()), 'kgdet_dcn_pack_weight_images: other bits than kgdet_dcn_pack_weight'
    for acc in (0, 1):
        base = torch.full_like(w, 0.5) if acc else None
        gw = Bytes(4 * w.numel(), base if acc else NAN)
        assert L.kgdet_dcn_unpack_weight_grad(ctypes.byref(s), P.packed.ptr(), gw.ptr(), ctypes.c_int(acc), _st()) == OK
        torch.cuda.synchronize()
        assert gw.intact() and P.untouched()
        assert torch.equal(gw.f32().reshape(w.shape), w + base if acc else w), 'unpack(pack(w)) is not w (accumulate %d)' % acc


# ------------------------------------------------------------------------------------------------ the head stage, grouped
CAT_KS = (3, 5, 7)
CAT_O = 16


def _cat_case(k):
    return (2, 16, 6, 7, CAT_O, k, 1, k // 2, 1, 1, 1)


def _cat_draw(seed):
    """the six-problem head stage of tests/test_gpu_dcn_edges.py: two maps [2, 16, 6, 7] x 3x3 / 5x5 / 7x7, the offsets of a kernel
    size shared by the maps, each map's three outputs windows of one [2, 48, 6, 7] buffer"""
    rng = np.random.default_rng(seed)
    xs = [rng.normal(size=(2, 16, 6, 7)).astype(np.float32) for _ in range(2)]
    offs = [E.edge_offsets(_cat_case(k), seed + k) for k in CAT_KS]
    ws = [[(rng.normal(size=(CAT_O, 16, k, k)) * 0.05).astype(np.float32) for k in CAT_KS] for _ in xs]
    gos = [rng.normal(size=(2, CAT_O * len(CAT_KS), 6, 7)).astype(np.float32) for _ in xs]
    return xs, offs, ws, gos


@functools.lru_cache(maxsize=None)
def _cat_ref():
    """per problem (map i, kernel j): the float64 oracle's y and gradients on the draw of SEED"""
    xs, offs, ws, gos = _cat_draw(SEED)
    f64 = lambda a: a.astype(np.float64)
    out = {}
    for i in range(2):
        for j, k in enumerate(CAT_KS):
            r = oracle.deform_conv_backward(f64(xs[i]), f64(offs[j]), f64(ws[i][j]), f64(gos[i][:, CAT_O * j:CAT_O * (j + 1)]), 1, k // 2, 1)
            r['y'] = oracle.deform_conv_forward(f64(xs[i]), f64(offs[j]), f64(ws[i][j]), 1, k // 2, 1)
            out[i, j] = r
    return out


class Stage(object):
    """the head stage on the device: six Problems that share the maps, offsets and grad_out buffers by POINTER, as dcn.py passes them"""

    def __init__(self, seed):
        xs, offs, ws, gos = _cat_draw(seed)
        self.P = []
        for i in range(2):
            for j, k in enumerate(CAT_KS):
                P = Problem(_cat_case(k), dict(x=xs[i], off=offs[j], w=ws[i][j], go=gos[i]), CAT_O * j, CAT_O * len(CAT_KS))
                if j > 0:
                    P.t['x'], P.t['go'] = self.P[3 * i].t['x'], self.P[3 * i].t['go']
                if i > 0:
                    P.t['off'] = self.P[j].t['off']
                self.P.append(P)
        self.n = len(self.P)
        self.shapes = (ctypes.POINTER(type(self.P[0].shape)) * self.n)(*[ctypes.pointer(P.shape) for P in self.P])

    def arr(self, ptrs):
        return (ctypes.c_void_p * self.n)(*[v.value if isinstance(v, ctypes.c_void_p) else v for v in ptrs])

    def ops(self, name):
        return self.arr([P.t[name].data_ptr() for P in self.P])

    def packs(self):
        return self.arr([P.packed.ptr() for P in self.P])


def _group_calls(S, R=None):
    n, ij = S.n, [(i, j) for i in range(2) for j in range(len(CAT_KS))]
    x_shape, y_shape = (2, 16, 6, 7), (2, CAT_O * len(CAT_KS), 6, 7)
    off_shape = lambda j: (2, 2 * CAT_KS[j] ** 2, 6, 7)
    w_shape = lambda j: (CAT_O, 16, CAT_KS[j], CAT_KS[j])
    cat = lambda name, i: np.concatenate([R[i, j][name] for j in range(len(CAT_KS))], 1)
    calls = []

    def add(name, outs, launch, refs, **kw):
        calls.append(Call('grouped ' + name, S.P, outs, launch, refs if R is not None else {}, **kw))
    add('forward', {'y%d' % i: (y_shape, NAN) for i in range(2)},
        lambda L, wp, wb, o: L.kgdet_deform_conv_forward_grouped(
            n, S.shapes, S.ops('x'), S.ops('off'), None, S.packs(), None, S.arr([o['y%d' % i] for i, j in ij]), ctypes.c_uint32(0),
            wp, wb, _st()),
        R and {'y%d' % i: (cat('y', i), 2e-5) for i in range(2)})
    # one grad_input per map and one grad_offset per offset tensor: the fix-up sums the problems that share a pointer, or the call
    # declines before it launches anything for that quantity (include/kgdet_hip.h) -- six problems of 9 / 25 / 49 stages get no
    # static schedule, dcn.py then takes the launch below
    add('backward_input, aliased sums', dict([('gi%d' % i, (x_shape, NAN)) for i in range(2)] +
                                             [('go%d' % j, (off_shape(j), NAN)) for j in range(len(CAT_KS))]),
        lambda L, wp, wb, o: L.kgdet_deform_conv_backward_input_grouped(
            n, S.shapes, S.ops('x'), S.ops('off'), S.packs(), S.ops('go'), S.arr([o['gi%d' % i] for i, j in ij]),
            S.arr([o['go%d' % j] for i, j in ij]), wp, wb, _st()),
        R and dict([('gi%d' % i, (sum(R[i, j]['grad_input'] for j in range(3)), GRAD_TOL)) for i in range(2)] +
                   [('go%d' % j, (sum(R[i, j]['grad_offset'] for i in range(2)), GRAD_TOL)) for j in range(3)]),
        declined=None, offset=True)
    add('backward_input, one output per problem', dict([('gi%d%d' % e, (x_shape, NAN)) for e in ij] +
                                                       [('go%d%d' % e, (off_shape(e[1]), NAN)) for e in ij]),
        lambda L, wp, wb, o: L.kgdet_deform_conv_backward_input_grouped(
            n, S.shapes, S.ops('x'), S.ops('off'), S.packs(), S.ops('go'), S.arr([o['gi%d%d' % e] for e in ij]),
            S.arr([o['go%d%d' % e] for e in ij]), wp, wb, _st()),
        R and dict([('gi%d%d' % e, (R[e]['grad_input'], GRAD_TOL)) for e in ij] +
                   [('go%d%d' % e, (R[e]['grad_offset'], GRAD_TOL)) for e in ij]),
        offset=True)
    for sched, option in (('', None), (', stream-K', OPT_WGRAD_STREAMK)):
        add('grad_weight' + sched, {'gw%d%d' % e: (w_shape(e[1]), NAN) for e in ij},
            lambda L, wp, wb, o: L.kgdet_deform_conv_grad_weight_grouped(
                n, S.shapes, S.ops('x'), S.ops('off'), S.ops('go'), S.arr([o['gw%d%d' % e] for e in ij]), wp, wb, _st()),
            R and {'gw%d%d' % e: (R[e]['grad_weight'], GRAD_TOL) for e in ij}, option=option)
    return calls


@functools.lru_cache(maxsize=None)
def _stages():
    return Stage(SEED), Stage(SEED + 1)


def _group_query(S):
    L = _L()
    query = L.kgdet_dcn_group_workspace_bytes(S.n, S.shapes)
    singles = [L.kgdet_dcn_workspace_bytes(ctypes.byref(P.shape)) for P in S.P]
    print('WS-QUERY head stage: kgdet_dcn_group_workspace_bytes %d, kgdet_dcn_workspace_bytes of the members %r' % (query, singles))
    assert query >= max(singles) > 0
    return query


def test_grouped_entry_points():
    """kgdet_deform_conv_forward_grouped, _backward_input_grouped (the aliased-sum attempt and the one-output-per-problem launch) and
    _grad_weight_grouped (output-stationary and stream-K) of the head stage on kgdet_dcn_group_workspace_bytes: (a) - (d)."""
    S, S1 = _stages()
    sizes = _sizes(_group_query(S))
    calls, twins = _group_calls(S, _cat_ref()), _group_calls(S1)
    # leftovers: forward <- grad_weight, the backward launches <- grad_weight (stream-K) / forward, grad_weight <- backward / forward
    for call, twin, other in zip(calls, twins, (3, 4, 0, 2, 0)):
        _contract(call, twin, calls[other], sizes, 'head stage')


def test_grouped_packers():
    """kgdet_dcn_pack_weight_multi of the six weights writes the images of six kgdet_dcn_pack_weight calls; the split images alone
    (kgdet_dcn_pack_weight_images 2, what training packs when kgdet_dcn_split_path_complete) serve the grouped forward with the same
    bits, the fp32 images left NaN."""
    L = _L()
    S, _ = _stages()
    multi = [Bytes(P.packed.size, NAN) for P in S.P]
    split = [Bytes(P.packed.size, NAN) for P in S.P]
    assert L.kgdet_dcn_pack_weight_multi(S.n, S.shapes, S.ops('w'), S.arr([b.ptr() for b in multi]), _st()) == OK
    assert L.kgdet_dcn_pack_weight_images(S.n, S.shapes, S.ops('w'), S.arr([b.ptr() for b in split]), ctypes.c_uint32(2), _st()) == OK
    torch.cuda.synchronize()
    for P, m, sp in zip(S.P, multi, split):
        assert m.intact() and sp.intact() and P.untouched()
        assert torch.equal(m.payload(), P.packed.payload()), 'kgdet_dcn_pack_weight_multi: other bits than kgdet_dcn_pack_weight'
    assert all(L.kgdet_dcn_split_path_complete(ctypes.byref(P.shape)) == 1 for P in S.P)
    ws = Bytes(_group_query(S))
    ys = []
    for packs in ([P.packed for P in S.P], split):
        y = [Bytes(4 * 2 * 48 * 6 * 7, NAN) for _ in range(2)]
        ws.payload().zero_()
        assert L.kgdet_deform_conv_forward_grouped(
            S.n, S.shapes, S.ops('x'), S.ops('off'), None, S.arr([b.ptr() for b in packs]), None,
            S.arr([y[i // 3].ptr() for i in range(S.n)]), ctypes.c_uint32(0), ws.ptr(), ctypes.c_size_t(ws.size), _st()) == OK
        torch.cuda.synchronize()
        assert ws.intact() and all(b.intact() for b in y + split)
        ys.append(y)
    for a, b in zip(*ys):
        assert bool(torch.isfinite(a.f32()).all()) and torch.equal(a.payload(), b.payload())


@pytest.mark.parametrize('member', range(6))
def test_group_query_serves_every_member(member):
    """include/kgdet_hip.h: kgdet_dcn_group_workspace_bytes is also >= kgdet_dcn_workspace_bytes of every member, "so the same
    buffer serves their backward calls" -- the v1 single-call entry points of each member (its output a channel window of the
    48-channel buffer) on the GROUP query: (a) - (d)."""
    S, S1 = _stages()
    i, j = divmod(member, 3)
    R = _cat_ref()[i, j]
    tag = 'member %d (map %d, %dx%d) ' % (member, i, CAT_KS[j], CAT_KS[j])
    calls = _single_calls(S.P[member], R, None, v2=False, tag=tag)
    twins = {c.name: c for c in _single_calls(S1.P[member], v2=False, tag=tag)}
    by_name = {c.name: c for c in calls}
    sizes = _sizes(_group_query(S))
    for call in calls:
        _contract(call, twins[call.name], _other_of(call.name, by_name, tag), sizes, 'head stage')


# --------------------------------------------------------------------------------------- 2. history of the Python route
def _leaves(*arrays):
    return [torch.from_numpy(np.array(a)).cuda().requires_grad_() for a in arrays]


def _cat_multi():
    from kgdet_amd import dcn
    xs, offs, ws, gos = _cat_draw(SEED)
    txs, tos = _leaves(*xs), _leaves(*offs)
    tws = [_leaves(*wl) for wl in ws]
    outs = dcn.deform_conv_cat_multi(txs, tos, tws, [k // 2 for k in CAT_KS], relu=False)
    torch.autograd.backward(outs, [_cuda(g) for g in gos])
    return [o.detach() for o in outs] + [t.grad for t in txs + tos + [w for wl in tws for w in wl]]


def _v1_autograd(case):
    from kgdet_amd import dcn
    N, C, H, W, O, k, s, p, d, g, dg = case
    r = _ref(case, False)
    tx, to, tw = _leaves(r['x'], r['off'], r['w'])
    y = dcn.deform_conv(tx, to, tw, s, p, d, g, dg)
    y.backward(_cuda(r['go']))
    return [y.detach(), tx.grad, to.grad, tw.grad]


def _dirty_the_workspace():
    """a 38 x 36 v2 forward + backward: grows the stream's workspace past every small query and leaves its tables in it"""
    from kgdet_amd import dcn
    case = E.LARGE_CASES[1]      # (its query, slabs + 3.8 MB, is above the head stage's group query, slabs + 2.7 MB)
    N, C, H, W, O, k, s, p, d, g, dg = case
    r = _ref(case, True)
    tx, to, tm, tw, tb = _leaves(r['x'], r['off'], r['mask'], r['w'], r['bias'])
    dcn.modulated_deform_conv(tx, to, tm, tw, tb, s, p, d, g, dg).backward(_cuda(r['go']))
    torch.cuda.synchronize()


@pytest.mark.parametrize('route', ['cat_multi', 'deform_conv'])
def test_python_route_does_not_depend_on_history(route, monkeypatch):
    """dcn.deform_conv_cat_multi on the head stage, and one v1 dcn.deform_conv autograd call on the first small case, forward +
    backward: with dcn._workspaces emptied (a fresh process: a new buffer of exactly the query) and after a 38 x 36 v2 call has grown
    and dirtied the workspace of the same stream -- every output and gradient bit for bit the same."""
    from kgdet_amd import dcn
    _L()
    run = _cat_multi if route == 'cat_multi' else functools.partial(_v1_autograd, E.SMALL_CASES[0])
    monkeypatch.setattr(dcn, '_workspaces', {})
    fresh = run()
    torch.cuda.synchronize()
    small = max(ws.numel() for ws in dcn._workspaces.values())
    monkeypatch.setattr(dcn, '_workspaces', {})
    _dirty_the_workspace()
    grown = max(ws.numel() for ws in dcn._workspaces.values())
    after = run()
    torch.cuda.synchronize()
    print('WS-HISTORY %s: fresh workspace %d bytes, grown %d bytes' % (route, small, grown))
    assert grown > small and max(ws.numel() for ws in dcn._workspaces.values()) == grown
    assert len(fresh) == len(after)
    for n, (a, b) in enumerate(zip(fresh, after)):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), '%s: result %d depends on the workspace\'s history' % (route, n)
