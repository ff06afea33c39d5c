"""Runs the cases of tests/psroi_edge_cases.py through kgdet_amd.deform_pool on the GPU.  Imported by
tests/test_gpu_psroi_edges.py for its own process (the default grad_data route: per-pixel contribution lists), and started by it
ONCE as a fresh process with KGDET_PSROI_GRAD_DATA=tiles -- csrc/psroi.hip reads that variable once per process -- to put every
case's backward on the tile-gather route:

    python tests/psroi_tiles_child.py OUT.npz

writes, per case, the gradients of the autograd run (`<case>/grad_data`, `<case>/grad_trans`), those of a second run through the
C ABI into NaN-filled outputs (`<case>/grad_data_abi`, `<case>/grad_trans_abi`) and kgdet_deform_psroi_backward_workspace_bytes
(`<case>/workspace`).  Not a test module."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from tests import psroi_edge_cases as E      # noqa: E402


def cuda(a, grad=False):
    t = torch.from_numpy(np.array(a)).cuda()
    return t.requires_grad_() if grad else t


def poison_allocator():
    """fill the caching allocator's free blocks, small pool and large pool, with NaN: whatever a kernel leaves unwritten shows"""
    junk = [torch.full((128 * 1024,), float('nan'), device='cuda') for _ in range(32)]
    junk += [torch.full((8 * 1024 * 1024,), float('nan'), device='cuda') for _ in range(4)]
    del junk


def op_args(case):
    c = case
    return (E.SCALE, c.pooled_size, c.out_dim, c.no_trans, c.group_size, c.part_size, c.sample_per_part, c.trans_std)


def autograd(case, r):
    """forward + backward through deform_roi_pooling: dict(out, count, grad_data, grad_trans (None with no_trans))"""
    from kgdet_amd.deform_pool import deform_roi_pooling
    td = cuda(r['data'], True)
    to = None if case.no_trans else cuda(r['offset'], True)
    out = deform_roi_pooling(td, cuda(r['rois']), td.new_empty(0) if case.no_trans else to, *op_args(case))
    count = out.grad_fn.output_count
    out.backward(cuda(r['grad_out']))
    return dict(out=out.detach(), count=count, grad_data=td.grad, grad_trans=None if case.no_trans else to.grad)


def shape_of(case):
    from kgdet_amd import _lib
    c = case
    s = _lib.PsroiShape()
    s.B, s.C, s.H, s.W, s.R = c.B, c.C, c.H, c.W, c.R
    s.out_dim, s.group_size, s.pooled_size, s.part_size, s.sample_per_part = (c.out_dim, c.group_size, c.pooled_size,
                                                                              c.part_size, c.sample_per_part)
    s.no_trans, s.num_classes = (1 if c.no_trans else 0), E.classes_of(c)
    s.spatial_scale, s.trans_std = E.SCALE, c.trans_std
    return s


def backward_workspace_bytes(case):
    from kgdet_amd import _lib
    return int(_lib.lib().kgdet_deform_psroi_backward_workspace_bytes(ctypes.byref(shape_of(case))))


def forward_abi(case, r):
    """kgdet_deform_psroi_forward into NaN-filled outputs: (out, count)"""
    from kgdet_amd import _lib
    c, L, shape = case, _lib.lib(), shape_of(case)
    td, tr = cuda(r['data']), cuda(r['rois'])
    to = None if c.no_trans else cuda(r['offset'])
    out = torch.full((c.R, c.out_dim, c.pooled_size, c.pooled_size), float('nan'), device='cuda')
    count = torch.full_like(out, float('nan'))
    ws_bytes = L.kgdet_deform_psroi_forward_workspace_bytes(ctypes.byref(shape))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    _lib.check(L.kgdet_deform_psroi_forward(ctypes.byref(shape), _lib.ptr(td), _lib.ptr(tr), _lib.ptr(to), _lib.ptr(out),
                                            _lib.ptr(count), _lib.ptr(ws), ctypes.c_size_t(ws_bytes), _lib.current_stream()),
               'kgdet_deform_psroi_forward')
    torch.cuda.synchronize()
    return out, count


def backward_abi(case, r, count):
    """kgdet_deform_psroi_backward into NaN-filled outputs: (grad_data, grad_trans (None with no_trans))"""
    from kgdet_amd import _lib
    c, L, shape = case, _lib.lib(), shape_of(case)
    td, tr, tg = cuda(r['data']), cuda(r['rois']), cuda(r['grad_out'])
    to = None if c.no_trans else cuda(r['offset'])
    gd = torch.full_like(td, float('nan'))
    gt = None if c.no_trans else torch.full_like(to, float('nan'))
    ws_bytes = L.kgdet_deform_psroi_backward_workspace_bytes(ctypes.byref(shape))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    _lib.check(L.kgdet_deform_psroi_backward(ctypes.byref(shape), _lib.ptr(tg), _lib.ptr(count), _lib.ptr(td), _lib.ptr(tr),
                                             _lib.ptr(to), _lib.ptr(gd), _lib.ptr(gt), _lib.ptr(ws), ctypes.c_size_t(ws_bytes),
                                             _lib.current_stream()), 'kgdet_deform_psroi_backward')
    torch.cuda.synchronize()
    return gd, gt


def main(path):
    assert os.environ.get('KGDET_PSROI_GRAD_DATA') == 'tiles', 'the child is there for the tile-gather route'
    assert torch.cuda.is_available(), 'GPU tests need a GPU (no fallback)'
    res = {}
    for case in E.CASES:
        r = E.reference(case)
        poison_allocator()
        a = autograd(case, r)
        poison_allocator()
        gd, gt = backward_abi(case, r, cuda(r['count32']))
        res[case.name + '/grad_data'] = a['grad_data'].cpu().numpy()
        res[case.name + '/grad_data_abi'] = gd.cpu().numpy()
        if not case.no_trans:
            res[case.name + '/grad_trans'] = a['grad_trans'].cpu().numpy()
            res[case.name + '/grad_trans_abi'] = gt.cpu().numpy()
        res[case.name + '/workspace'] = np.int64(backward_workspace_bytes(case))
    np.savez(path, **res)


if __name__ == '__main__':
    main(sys.argv[1])
