"""The table of tests/dcn_group_cases.py held on the CPU: the float64 oracle against the independent grid_sample formulation
(tests/torch_ref.py) under float64 autograd, the float32 oracle against the float64 one at the GPU tolerances (so those bars can be
met by correct fp32 arithmetic on these inputs), and the routing facts the ids and docstrings of tests/test_gpu_dcn_groups.py
quote, recomputed from the definitions of csrc/dcn_api.hip and checked against the constants in the kernel sources."""
import os
import re

import numpy as np
import pytest
import torch

from tests import dcn_group_cases as G
from tests import torch_ref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'kgdet_amd', 'csrc')
AGREE = 1e-12           # oracle against grid_sample, both float64 (measured: 4e-15 or better)
FORWARD_TOL = 2e-5      # the GPU bars of tests/test_gpu_dcn_groups.py
GRAD_TOL = 5e-5


def _rel(a, b):
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-300)


def _torch_ref(r, case, v2):
    N, C, H, W, O, k, s, p, d, g, dg = case
    t = lambda a, grad=True: None if a is None else torch.from_numpy(np.array(a, np.float64)).requires_grad_(grad)
    x, off, w, mask, bias = (t(r[n]) for n in ('x', 'off', 'w', 'mask', 'bias'))
    y = torch_ref.deform_conv(x, off, w, stride=s, padding=p, dilation=d, groups=g, deformable_groups=dg, mask=mask, bias=bias)
    y.backward(t(r['go'], False))
    out = dict(y=y.detach(), grad_input=x.grad, grad_offset=off.grad, grad_weight=w.grad)
    if v2:
        out.update(grad_mask=mask.grad, grad_bias=bias.grad)
    return {n: v.numpy() for n, v in out.items()}


@pytest.mark.parametrize('v2', [False, True], ids=['v1', 'v2'])
@pytest.mark.parametrize('case', G.CASES, ids=G.case_id)
def test_float64_oracle_agrees_with_grid_sample(case, v2):
    r = G.reference(case, v2)
    want = _torch_ref(r, case, v2)
    for name in ('y',) + G.grads(v2):
        assert r[name].shape == want[name].shape, name
        err = _rel(r[name], want[name])
        assert err < AGREE, '%s %s: %.3e' % (G.case_id(case), name, err)


@pytest.mark.parametrize('v2', [False, True], ids=['v1', 'v2'])
@pytest.mark.parametrize('case', G.CASES, ids=G.case_id)
def test_float32_oracle_meets_the_gpu_bars(case, v2):
    r = G.reference(case, v2)
    r32 = G.compute(r, case, v2, np.float32)
    for name in ('y',) + G.grads(v2):
        assert r32[name].dtype == np.float32
        err, tol = _rel(r32[name].astype(np.float64), r[name]), FORWARD_TOL if name == 'y' else GRAD_TOL
        assert err < tol, '%s %s: %.3e (bar %.1e)' % (G.case_id(case), name, err, tol)


def test_reference_is_cached_and_read_only():
    case = G.BY_NAME['8x4']
    r = G.reference(case, True)
    assert r is G.reference(case, True)
    for name, a in r.items():
        assert not a.flags.writeable, name
    assert r['x'].dtype == np.float32 and r['y'].dtype == np.float64
    assert set(G.grads(True)) <= set(r) and G.reference(case, False)['mask'] is None


def _constant(header, pattern):
    # (a space in `pattern` stands for any run of white space, line breaks included: a reformatted line still matches)
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(pattern.replace(' ', r'\s*'), f.read())
    assert m, (header, pattern)
    return m


def test_constants_are_those_of_the_kernel_sources():
    for name, want in (('kChunk', G.CHUNK), ('kTileM', G.TILE_M), ('kMaxFwdGroup', G.MAX_RUNS), ('kPlaneMaxHW', G.PLANE_MAX_HW)):
        assert int(_constant('dcn_common.h', r'constexpr int %s = (\d+);' % name).group(1)) == want, name
    m = _constant('dcn_api.hip', r's->H \* s->W <= (\d+) \* (\d+) && dg_ok')        # plan_bwd_lds
    assert int(m.group(1)) * int(m.group(2)) == G.EXACT_MAX_HW
    _constant('dcn_api.hip', r'd\.Cg_pad = \(int\)align_up\(d\.Cg, kChunk\);')
    _constant('dcn_api.hip', r'd\.Og_pad = \(int\)align_up\(d\.Og, kTileM\);')
    _constant('dcn_api.hip', r'if \(n_runs > kMaxFwdGroup\) return false;')          # plane_bwd_input_ok


def test_facts_of_the_table():
    f = {name: G.facts(case) for name, case in G.RESNEXT + G.MIXED}
    # (Cg, Og) per case, as the table's names say
    want = {'8x4': (4, 4), '8x4-stride2': (4, 4), '9x4': (4, 4), '32x4': (4, 4), '32x8-stride2': (8, 8), '32x16': (16, 16),
            '32x32': (32, 32), '8x1-depthwise': (1, 1), '8x2-Og6': (2, 6), '8x6-Og3': (6, 3), '8x4-5x5': (4, 4),
            '8x4-1200px': (4, 4), '8x4-1368px': (4, 4), '32x4-1368px': (4, 4), '8x1-1368px': (1, 1),
            '8x4-dg8': (4, 4), '8x8-dg2': (8, 8), '2x32-dg8': (32, 32)}
    assert {n: (v['Cg'], v['Og']) for n, v in f.items()} == want
    # channel runs: the 8-group cases sit exactly on the limit of the plane grad_input kernel, 9 and 32 groups beyond it
    for name, case in G.RESNEXT:
        assert f[name]['n_runs'] == case[9], name
        assert f[name]['plane_grad_input'] == (case[9] <= G.MAX_RUNS and f[name]['map_class'] != 'large'), name
    assert [n for n, _ in G.RESNEXT if f[n]['n_runs'] == G.MAX_RUNS and f[n]['plane_grad_input']] == \
        ['8x4', '8x4-stride2', '8x1-depthwise', '8x2-Og6', '8x6-Og3', '8x4-5x5', '8x4-1200px']
    assert f['9x4']['n_runs'] == G.MAX_RUNS + 1 and not f['9x4']['plane_grad_input']
    assert f['32x4']['n_runs'] == 32
    # the runs tile the channels, each inside one weight group and one deformable group
    for case in G.CASES:
        N, C, H, W, O, k, s, p, d, g, dg = case
        runs = G.channel_runs(case)
        assert runs[0][0] == 0 and runs[-1][1] == C and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
        for c0, c1, gi, di in runs:
            assert gi * (C // g) <= c0 < c1 <= (gi + 1) * (C // g) and di * (C // dg) <= c0 < c1 <= (di + 1) * (C // dg)
    assert f['8x4-dg8']['n_runs'] == 8 and f['8x8-dg2']['n_runs'] == 8 and f['2x32-dg8']['n_runs'] == 8
    assert f['8x4-dg8']['cpdg'] == 4 and f['8x8-dg2']['cpdg'] == 32 and f['2x32-dg8']['cpdg'] == 8
    # every map class is hit, and by the cases the table names
    assert {v['map_class'] for v in f.values()} == {'lds', 'plane', 'large'}
    assert [n for n, v in f.items() if v['map_class'] == 'plane'] == ['8x4-1200px']
    assert [n for n, v in f.items() if v['map_class'] == 'large'] == ['8x4-1368px', '32x4-1368px', '8x1-1368px']
    assert G.EXACT_MAX_HW < 30 * 40 <= G.PLANE_MAX_HW < 38 * 36
    # backward_input: the maps beyond plan_bwd_lds' 1088 pixels take the zero-padded large-map route (Og % 16 != 0, and with Cg = 1
    # an odd K * Cg as well: input channels padded too), every other ResNeXt case dcn_bwd_input_gather
    padded = ['8x4-1200px', '8x4-1368px', '32x4-1368px', '8x1-1368px']
    assert [n for n, _ in G.RESNEXT if f[n]['backward_input_route'] == 'large-padded'] == padded
    assert all(f[n]['backward_input_route'] == 'gather' for n, _ in G.RESNEXT if n not in padded)
    assert all(f[n]['Og'] % G.LARGE_OG_MULTIPLE != 0 for n in padded)
    assert all(f[n]['backward_input_route'] is None for n, _ in G.MIXED)
    _constant('dcn_backward_large.hip', r'return p\.Og % 16 == 0 && \(\(long long\)p\.K \* p\.C_total\) % 2 == 0')
    assert [n for n, v in f.items() if v['taps_times_channels_odd']] == ['8x1-depthwise', '8x1-1368px']
    # padding: with Cg = Og = 4, 3/4 of a reduction chunk and 63/64 of a row tile
    assert (f['32x4']['Cg_pad'], f['32x4']['Og_pad'], f['32x4']['Og_pad16']) == (16, 256, 16)
    assert f['32x16']['Cg_pad'] == 16 and f['32x32']['Cg_pad'] == 32 and f['8x6-Og3']['Cg_pad'] == 16
    # 'exact' arithmetic: one 32-channel slice per group everywhere (never run with Cg < 32 before this table)
    assert all(v['exact_slices'] == case[9] for (n, case), v in zip(G.RESNEXT + G.MIXED, f.values()))
    # 5x5: 25 taps
    assert f['8x4-5x5']['K'] == 25
    # the subsets
    assert [G.NAMES[c] for c in G.GUARDED] == ['8x4', '32x4', '8x1-depthwise', '8x6-Og3', '32x4-1368px']
    assert len(set(G.CASES)) == len(G.CASES) == 18
