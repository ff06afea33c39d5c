"""``kgdet_jpeg_encode`` / ``kgdet_jpeg_write`` (csrc/jpeg.hip) through the C ABI.

The bar is EQUALITY of bytes and lengths with ``jpeg.jpeg_restatement`` (held to a float64 reference, a parser and PIL's decoder
on the CPU by tests/test_jpeg_refs.py).  Output and workspace are pre-filled with 0xA5 and sit between 64-byte canaries: every
byte of a file must be written, nothing beside it -- not even inside a capacity larger than the file -- and the source must
come back unchanged."""
import ctypes

import numpy as np
import pytest
import torch

from kgdet_amd import _lib, jpeg
from tests import jpeg_refs as jr

pytestmark = pytest.mark.gpu
i32, i64, vp, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
FILL, CANARY, PAD = 0xA5, 0x5C, 64
SLACK = 7                    # bytes of capacity beyond the file: they must stay as they were


class Call(object):
    """one ``kgdet_jpeg_encode`` + ``kgdet_jpeg_write`` of ``images`` at ``quality``; image i lies at an odd offset of the source
    buffer, in list order or (``reverse``) in reverse order, and its file goes to ``out`` in list order"""

    def __init__(self, images, quality=90, reverse=False):
        self.images, self.n, self.quality = images, len(images), quality
        order = list(range(self.n))[::-1] if reverse else list(range(self.n))
        self.src_at, total = [0] * self.n, 3
        for i in order:
            self.src_at[i] = total
            total += images[i].size + 5
        self.src_host = np.full(total, 0x33, dtype=np.uint8)
        for img, at in zip(images, self.src_at):
            self.src_host[at:at + img.size] = img.reshape(-1)
        self.src = torch.from_numpy(self.src_host).cuda()
        self.out_at = [0] * self.n
        self.table = self.make_table()
        self.ws_bytes = _lib.lib().kgdet_jpeg_workspace_bytes(self.table, i32(self.n))
        self.ws_all = torch.full((self.ws_bytes + 2 * PAD,), FILL, dtype=torch.uint8, device='cuda')
        self.ws_all[:PAD] = CANARY
        self.ws_all[PAD + self.ws_bytes:] = CANARY
        self.ws = self.ws_all[PAD:PAD + self.ws_bytes]
        self.lengths = torch.full((self.n + 2,), -7, dtype=torch.int64, device='cuda')
        self.out = self.status = None

    def make_table(self):
        return (i64 * (4 * self.n))(*[v for i in range(self.n) for v in (self.src_at[i], self.out_at[i], self.images[i].shape[0],
                                                                          self.images[i].shape[1])])

    def encode(self, **override):
        a = dict(src=_lib.ptr(self.src), src_bytes=self.src.numel(), table=self.table, n=self.n, quality=self.quality,
                 ws=_lib.ptr(self.ws), ws_bytes=self.ws_bytes, lengths=vp(self.lengths.data_ptr() + 8))
        a.update(override)
        rc = _lib.lib().kgdet_jpeg_encode(a['src'], i64(a['src_bytes']), a['table'], i32(a['n']), i32(a['quality']), a['ws'],
                                          sz(a['ws_bytes']), a['lengths'], _lib.current_stream())
        torch.cuda.synchronize()
        return rc

    def reported(self):
        host = self.lengths.cpu().numpy()
        assert host[0] == -7 and host[-1] == -7, 'written beside the lengths'
        return [int(v) for v in host[1:-1]]

    def prepare_out(self, sizes, slack=SLACK):
        """the output buffer: canary, then per image its capacity of ``sizes[i] + slack`` bytes and a gap of 3 bytes, canary"""
        total = PAD
        self.capacity = []
        for i, size in enumerate(sizes):
            self.out_at[i] = total
            self.capacity.append(max(size + slack, 0))
            total += self.capacity[-1] + 3
        self.table = self.make_table()
        self.out = torch.full((total + PAD,), FILL, dtype=torch.uint8, device='cuda')
        self.out[:PAD] = CANARY
        self.out[-PAD:] = CANARY
        self.status = torch.full((self.n + 2,), -7, dtype=torch.int32, device='cuda')

    def write(self, **override):
        a = dict(table=self.table, n=self.n, quality=self.quality, ws=_lib.ptr(self.ws), ws_bytes=self.ws_bytes,
                 capacity=(i64 * self.n)(*self.capacity), out=_lib.ptr(self.out), out_bytes=self.out.numel(),
                 status=vp(self.status.data_ptr() + 4))
        a.update(override)
        rc = _lib.lib().kgdet_jpeg_write(a['table'], i32(a['n']), i32(a['quality']), a['ws'], sz(a['ws_bytes']), a['capacity'],
                                         a['out'], i64(a['out_bytes']), a['status'], _lib.current_stream())
        torch.cuda.synchronize()
        return rc

    def files(self, sizes):
        """the files as written; asserts the canaries, every byte outside the files, the workspace's canaries and the source"""
        host = self.out.cpu().numpy()
        assert (host[:PAD] == CANARY).all() and (host[-PAD:] == CANARY).all(), 'a canary of the output was overwritten'
        mask = np.ones(host.size, dtype=bool)
        mask[:PAD] = mask[-PAD:] = False
        got = []
        for at, size in zip(self.out_at, sizes):
            mask[at:at + size] = False
            got.append(host[at:at + size].tobytes())
        assert (host[mask] == FILL).all(), 'bytes beside the files were written'
        self.untouched_around()
        return got

    def untouched_around(self):
        ws = self.ws_all.cpu().numpy()
        assert (ws[:PAD] == CANARY).all() and (ws[PAD + self.ws_bytes:] == CANARY).all(), 'a canary of the workspace was overwritten'
        assert np.array_equal(self.src.cpu().numpy(), self.src_host), 'the source was written'

    def run(self):
        """both calls -> (lengths, files, status)"""
        assert self.encode() == 0, _lib.lib().kgdet_last_error()
        sizes = self.reported()
        self.prepare_out(sizes)
        assert self.write() == 0, _lib.lib().kgdet_last_error()
        status = self.status.cpu().numpy()
        assert status[0] == -7 and status[-1] == -7, 'written beside the status'
        return sizes, self.files(sizes), status[1:-1].tolist()


def check(names, quality=90, reverse=False):
    images = [np.ascontiguousarray(jr.image(name)) for name in names]
    sizes, files, status = Call(images, quality, reverse).run()
    for name, size, data in zip(names, sizes, files):
        want = jr.restated(name, quality)['bytes']
        assert size == len(want), '%s q%d: %d bytes reported, the restatement has %d' % (name, quality, size, len(want))
        if data != want:
            first = next(k for k in range(len(want)) if data[k] != want[k])
            raise AssertionError('%s q%d: first difference at byte %d of %d (header %d)' % (name, quality, first, len(want),
                                                                                           jpeg.HEADER_BYTES))
    assert status == [0] * len(names)
    return files


@pytest.mark.parametrize('name,quality', jr.RUNS)
def test_every_case_and_quality_equals_the_restatement(name, quality):
    check([name], quality)


def test_three_sizes_in_one_call_in_table_order_and_reversed():
    names = ['noise-17x9', 'ramp-80x96', 'noise-112x96']
    assert check(names) == check(names, reverse=True) == [jr.restated(n, 90)['bytes'] for n in names]


def test_thirty_two_images_of_one_mcu():
    names = ['noise-16x16', 'grey-16x16', 'checker-16x16', 'noise-16x16'] * 8
    assert len(names) == jpeg.MAX_IMAGES
    check(names, 100)


def test_the_multi_range_case_twice_gives_identical_bytes():
    assert len(jr.restated(jr.MULTI_RANGE, 90)['stream']) > 2 * jpeg.RANGE_BYTES
    assert check([jr.MULTI_RANGE]) == check([jr.MULTI_RANGE])


def test_refusals_return_shape_errors_and_write_nothing():
    img = np.ascontiguousarray(jr.image('noise-17x9'))
    H, W = img.shape[:2]
    null = vp(0)
    want = jr.restated('noise-17x9', 90)['bytes']

    def tab(*row):
        return (i64 * 4)(*row)
    call = Call([img])
    at = call.src_at[0]
    cases = [dict(n=-1), dict(n=33), dict(quality=0), dict(quality=101), dict(table=tab(at, 0, 0, W)), dict(table=tab(at, 0, H, 0)),
             dict(table=tab(at, 0, 8193, 1)), dict(table=tab(at, 0, 1, 8193)), dict(table=tab(-1, 0, H, W)),
             dict(table=tab(at + 6, 0, H, W)), dict(src_bytes=-1), dict(src_bytes=at + img.size - 1), dict(src=null), dict(table=null),
             dict(ws=null), dict(lengths=null), dict(ws=vp(call.ws.data_ptr() + 8)),
             dict(src=_lib.ptr(call.ws), src_bytes=call.ws_bytes),                                  # source = workspace
             dict(lengths=vp(call.ws.data_ptr() + 64)),                                             # lengths inside the workspace
             dict(lengths=vp(call.src.data_ptr() + 8))]                                             # lengths inside the source
    for kw in cases:
        assert call.encode(**kw) == _lib.KGDET_E_SHAPE, kw
        assert (call.ws_all[PAD:PAD + call.ws_bytes] == FILL).all() and call.reported() == [-7], kw
        call.untouched_around()
    assert call.encode(ws_bytes=call.ws_bytes - 1) == _lib.KGDET_E_WORKSPACE and (call.ws == FILL).all()
    assert call.encode(n=0, table=null, src=null, ws=null, lengths=null) == 0 and (call.ws == FILL).all()
    assert _lib.lib().kgdet_jpeg_workspace_bytes(tab(0, 0, 0, W), i32(1)) == 0
    assert _lib.lib().kgdet_jpeg_workspace_bytes(tab(0, 0, H, W), i32(33)) == 0
    assert call.encode() == 0 and call.reported() == [len(want)]
    call.prepare_out([len(want)])
    o = call.out_at[0]
    cases = [dict(n=-1), dict(n=33), dict(quality=0), dict(quality=101), dict(table=tab(at, o, 0, W)), dict(table=tab(at, o, H, 8193)),
             dict(table=tab(at, -1, H, W)), dict(table=tab(at, call.out.numel() - len(want), H, W)), dict(capacity=(i64 * 1)(-1)),
             dict(out_bytes=-1), dict(out_bytes=o + len(want) - 1), dict(table=null), dict(ws=null), dict(capacity=null),
             dict(out=null), dict(status=null), dict(ws=vp(call.ws.data_ptr() + 8)),
             dict(out=_lib.ptr(call.ws), out_bytes=call.ws_bytes),                                  # output = workspace
             dict(status=vp(call.ws.data_ptr() + 64)),                                              # status inside the workspace
             dict(status=vp(call.out.data_ptr() + 8))]                                              # status inside the output
    for kw in cases:
        assert call.write(**kw) == _lib.KGDET_E_SHAPE, kw
        assert call.files([0]) == [b''] and (call.status == -7).all(), kw
    assert call.write(ws_bytes=call.ws_bytes - 1) == _lib.KGDET_E_WORKSPACE and call.files([0]) == [b'']
    assert call.write(n=0, table=null, ws=null, capacity=null, out=null, status=null) == 0 and call.files([0]) == [b'']
    assert call.write() == 0 and call.files([len(want)]) == [want]
    two = Call([img, img])                                                                          # two files that overlap
    assert two.encode() == 0
    two.prepare_out(two.reported())
    two.out_at[1] = two.out_at[0] + len(want) - 1
    two.table = two.make_table()
    assert two.write() == _lib.KGDET_E_SHAPE and two.files([0, 0]) == [b'', b'']


def test_an_output_one_byte_too_small_is_reported_and_not_written():
    names = ['noise-17x9', 'noise-80x96', 'ramp-24x40']
    call = Call([np.ascontiguousarray(jr.image(name)) for name in names])
    assert call.encode() == 0
    sizes = call.reported()
    assert sizes == [len(jr.restated(name, 90)['bytes']) for name in names]
    call.prepare_out([sizes[0], sizes[1] - 1, sizes[2]], slack=0)
    assert call.write() == 0, _lib.lib().kgdet_last_error()
    assert call.status.cpu().numpy()[1:-1].tolist() == [0, 1, 0]
    got = call.files([sizes[0], 0, sizes[2]])
    assert got[0] == jr.restated(names[0], 90)['bytes'] and got[2] == jr.restated(names[2], 90)['bytes']
