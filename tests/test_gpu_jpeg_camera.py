"""``kgdet_jpeg_decode_camera`` (csrc/jpeg_decode.hip) through the C ABI and ``jpeg.DeviceJpegDecoder(camera=True)``: 4:2:2 files
and restart intervals.

The bar is EQUALITY of every byte of the picture with ``jpeg.decode_restatement(data, camera=True)`` (held to PIL's decoder on
the CPU by tests/test_jpeg_camera_refs.py), and with ``kgdet_jpeg_decode`` for the files that entry point takes.  Buffers are
laid out and pre-filled as in tests/test_gpu_jpeg_decode.py: 0xA5 between 64-byte canaries, odd offsets, gaps.  The malformed
files are inputs the kernels are specified to survive: their status words and the canaries are what is checked."""
import ctypes

import numpy as np
import pytest
import torch

from kgdet_amd import _lib, jpeg
from tests import jpeg_camera_refs as cr
from tests import jpeg_decode_refs as dr
from tests.test_gpu_jpeg_decode import CANARY, FILL, PAD, Call

pytestmark = pytest.mark.gpu
i32, i64, vp, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
NOT_EOI, BAD_SCAN, BAD_RESTART = 2, 3, 4


class CameraCall(Call):
    """one ``kgdet_jpeg_decode_camera`` of ``files`` (``old=True``: one ``kgdet_jpeg_decode``), laid out as ``Call`` does"""

    def __init__(self, files, old=False, intervals=None):
        self.files, self.n, self.old = files, len(files), old
        self.frames = [jpeg.parse_header(f, camera=not old) for f in files]
        assert not any(isinstance(f, str) for f in self.frames), self.frames
        self.intervals = [f.get('restart_interval', 0) for f in self.frames] if intervals is None else intervals
        at, self.places = 3, []
        for data, frame in zip(files, self.frames):
            scan = len(data) - frame['scan_offset']
            self.places.append((at, scan, at + scan + 7))
            at += scan + 7 + jpeg.DECODE_TABLE_BYTES + 2
        self.src_host = np.full(at, 0x33, dtype=np.uint8)
        for data, frame, (so, sb, to) in zip(files, self.frames, self.places):
            self.src_host[so:so + sb] = np.frombuffer(data, dtype=np.uint8, offset=frame['scan_offset'])
            self.src_host[to:to + jpeg.DECODE_TABLE_BYTES] = np.frombuffer(frame['tables'], dtype=np.uint8)
        self.src = torch.from_numpy(self.src_host).cuda()
        self.out_at, total = [], PAD + 1
        for frame in self.frames:
            self.out_at.append(total)
            total += 3 * frame['H'] * frame['W'] + 5
        self.out = torch.full((total + PAD,), FILL, dtype=torch.uint8, device='cuda')
        self.out[:PAD] = CANARY
        self.out[-PAD:] = CANARY
        self.jobs = self.make_jobs()
        self.ws_bytes = self.workspace_bytes(self.jobs, i32(self.n))
        assert self.ws_bytes > 0
        self.ws_all = torch.full((self.ws_bytes + 2 * PAD,), FILL, dtype=torch.uint8, device='cuda')
        self.ws_all[:PAD] = CANARY
        self.ws_all[PAD + self.ws_bytes:] = CANARY
        self.ws = self.ws_all[PAD:PAD + self.ws_bytes]
        self.status = torch.full((self.n + 2,), -7, dtype=torch.int32, device='cuda')

    @property
    def workspace_bytes(self):
        L = _lib.lib()
        return L.kgdet_jpeg_decode_workspace_bytes if self.old else L.kgdet_jpeg_decode_camera_workspace_bytes

    def make_jobs(self, **change):
        rows = [dict(scan_offset=so, scan_bytes=sb, tables_offset=to, dst_offset=at, H=f['H'], W=f['W'], mode=f['mode'], reserved=r)
                for (so, sb, to), at, f, r in zip(self.places, self.out_at, self.frames, self.intervals)]
        for field, (i, value) in change.items():
            rows[i][field] = value
        return (_lib.JpegDecodeJob * max(self.n, 1))(*[_lib.JpegDecodeJob(**r) for r in rows])

    def decode(self, **override):
        a = dict(src=_lib.ptr(self.src), src_bytes=self.src.numel(), jobs=self.jobs, n=self.n, ws=_lib.ptr(self.ws),
                 ws_bytes=self.ws_bytes, out=_lib.ptr(self.out), out_bytes=self.out.numel(), status=vp(self.status.data_ptr() + 4))
        a.update(override)
        fn = _lib.lib().kgdet_jpeg_decode if self.old else _lib.lib().kgdet_jpeg_decode_camera
        rc = fn(a['src'], i64(a['src_bytes']), a['jobs'], i32(a['n']), a['ws'], sz(a['ws_bytes']), a['out'], i64(a['out_bytes']),
                a['status'], _lib.current_stream())
        torch.cuda.synchronize()
        return rc

    def header(self):
        """(stream lengths, rounds) of the workspace header"""
        words = self.ws[:256].view(torch.int32).cpu().tolist()
        return words[:self.n], words[32:32 + self.n]


def check(files, expected=None):
    """one camera call of ``files`` -> the call; every picture equals the definition's"""
    call = CameraCall(files)
    for k, (data, got) in enumerate(zip(files, call.run())):
        want = jpeg.decode_restatement(data, camera=True) if expected is None else expected[k]
        assert got.shape == want.shape and np.array_equal(got, want), k
    return call


# ---- 4:2:2 ---------------------------------------------------------------------------------------------------------------------
WIDTHS_422, HEIGHTS_422 = (1, 5, 11, 15, 16, 17, 21, 31, 33), (1, 7, 8, 9, 17)


def test_422_files_of_every_edge_size_equal_the_restatement_beside_the_other_modes():
    cases = [(('noise', 'ramp')[(i + j) % 2], H, W, (90, 50, 100)[(i + j) % 3], '422', None, bool((i + j) % 2))
             for i, H in enumerate(HEIGHTS_422) for j, W in enumerate(WIDTHS_422)]
    assert len(cases) == 45
    others = [('noise', 17, 33, 90, '420', None, False), ('ramp', 9, 21, 50, '444', None, False), ('noise', 17, 31, 90, 'grey', None, False),
              ('noise', 9, 3, 90, '422', None, False), ('noise', 9, 4, 90, '422', None, False)]       # (and the two-sample chroma rows)
    for part in (cases[:20] + others, cases[20:] + others[:3]):      # two calls, each with all four modes
        files = [cr.make(*c) for c in part]
        assert len(files) <= 32 and {cr.frame_of(f)['mode'] for f in files} == {0, 1, 2, 3}
        call = check(files, [cr.restated(c) for c in part])
        for data, got in zip(files, call.pictures()):
            assert np.array_equal(got, dr.pil(data))


# ---- restart intervals -----------------------------------------------------------------------------------------------------------
def test_restart_files_of_every_mode_and_interval_equal_the_restatement():
    cases = []
    for kind, (H, W) in (('420', (40, 56)), ('422', (23, 49)), ('444', (33, 49)), ('grey', (33, 49))):
        mw = jpeg.frame_blocks(cr.frame_of(cr.make('noise', H, W, 90, kind)))[0]
        assert mw % 3 != 0                                      # an interval of 3 does not divide the MCUs of a row
        for restart in (('blocks', 1), ('blocks', 2), ('blocks', 3), ('rows', 1), ('rows', 2), ('blocks', 1000)):
            cases.append((('noise', 'ramp')[len(cases) % 2], H, W, (90, 100, 30)[len(cases) % 3], kind, restart, len(cases) % 4 == 3))
    files = [cr.make(*c) for c in cases]
    assert len(files) == 24 and all(cr.frame_of(f)['restart_interval'] > 0 for f in files)
    call = check(files, [cr.restated(c) for c in cases])
    for data, got in zip(files, call.pictures()):
        assert np.array_equal(got, dr.pil(data))
    again = CameraCall(files)                                   # repeatability: two calls give equal bits
    assert all(np.array_equal(a, b) for a, b in zip(again.run(), call.pictures()))
    assert again.header() == call.header()


def test_many_short_intervals_share_a_subsequence():
    """a white one-component file with interval 1: every interval codes its DC value from 0 and an EOB, three bytes with PIL's
    tables, so the 64 interval starts lie in three subsequences; every lane of the kernel holds an interval start"""
    data = cr.make('uniform', 64, 64, 90, 'grey', ('blocks', 1))
    parts = jpeg.decode_parts(data, camera=True)
    assert len(parts['intervals']) == 64 and set(parts['intervals']) == {3}
    assert 8 * len(parts['stream']) == 3 * jpeg.DECODE_SUBSEQ_BITS
    call = check([data], [parts['image']])
    assert np.array_equal(call.pictures()[0], dr.pil(data))
    assert call.header() == ([len(parts['stream'])], [1])        # every lane holds an interval start: one round


def test_more_intervals_than_a_chunk_has_lanes():
    data = cr.make('noise', 264, 264, 90, '444', ('blocks', 1))
    parts = jpeg.decode_parts(data, camera=True)
    assert len(parts['intervals']) == 1089 > jpeg.DECODE_CHUNK_LANES
    call = check([data], [parts['image']])
    assert np.array_equal(call.pictures()[0], dr.pil(data))


def test_a_single_interval_longer_than_a_chunk():
    data = cr.make('noise', 256, 256, 100, '444', ('blocks', 1024))
    assert cr.frame_of(data)['restart_interval'] == 1024 and cr.markers(data) == []
    call = check([data])
    lengths, rounds = call.header()
    assert lengths[0] > jpeg.DECODE_CHUNK_LANES * jpeg.DECODE_SUBSEQ_BITS // 8, lengths      # read from the workspace header
    assert np.array_equal(call.pictures()[0], dr.pil(data))
    two = cr.make('noise', 256, 256, 100, '444', ('rows', 16))    # and two intervals of that length: two workgroups
    assert len(cr.markers(two)) == 1
    call = check([two, data])
    assert min(call.header()[0]) > jpeg.DECODE_CHUNK_LANES * jpeg.DECODE_SUBSEQ_BITS // 8


def test_a_uniform_picture_with_one_row_intervals_takes_the_rounds_of_its_longest_interval():
    data = cr.make('uniform', 624, 468, 90, '420', ('rows', 1))
    parts = jpeg.decode_parts(data, camera=True)
    call = check([data], [parts['image']])
    _, rounds = call.header()
    longest = -(-8 * max(parts['intervals']) // jpeg.DECODE_SUBSEQ_BITS)
    print('rounds %s, subsequences of the longest interval %d' % (rounds, longest))
    assert 1 <= rounds[0] <= longest + 1


# ---- the old entry point ----------------------------------------------------------------------------------------------------------
def test_files_the_old_entry_point_takes_give_equal_bytes_from_both():
    files = [dr.make(*case) for case in dr.GPU_CASES[3::5][:29]] + [dr.demo_file(), dr.make(*dr.UNIFORM_CASES[0]), dr.make(*dr.LONG_CASE)]
    assert len(files) == 32 and len({jpeg.parse_header(f)['mode'] for f in files}) == 3
    new, old = CameraCall(files), CameraCall(files, old=True)
    for k, (a, b) in enumerate(zip(new.run(), old.run())):
        assert np.array_equal(a, b), k
    assert new.header() == old.header()                         # the same stream lengths and the same rounds
    assert new.ws_bytes > old.ws_bytes


# ---- statuses -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['420', '422', 'grey'])
def test_a_malformed_restart_file_gets_its_status_and_touches_nothing_else(kind):
    good = cr.make('noise', 40, 56, 90, kind, ('blocks', 2))
    bad = cr.broken(good)
    neighbours = [cr.make('ramp', 33, 47, 50, '422', ('rows', 1)), dr.make('checker', 33, 47, 50, '420')]
    names = sorted(bad)
    files = [neighbours[0]] + [bad[name] for name in names] + [neighbours[1]]
    frames = [cr.frame_of(f) for f in files]
    call = CameraCall(files)
    assert call.decode() == 0, _lib.lib().kgdet_last_error()
    status = call.verdicts()
    # an interval cut short at its tail is BAD_RESTART: the true parse stops in front of the symbol that no longer fits
    assert status == [0] + [BAD_RESTART] * len(names) + [0], list(zip(names, status[1:-1]))
    got = call.pictures()
    assert np.array_equal(got[0], dr.pil(neighbours[0])) and np.array_equal(got[-1], dr.pil(neighbours[1]))
    assert all(f['restart_interval'] == 2 for f in frames[1:-1])


def test_a_restart_marker_with_interval_0_is_not_eoi_and_an_invalid_code_is_bad_scan():
    good = cr.make('noise', 40, 56, 90, '420', ('blocks', 2))
    plain = dr.make('noise', 33, 47, 90, '420')
    start = dr.scan_start(plain)
    middle = start + (len(plain) - start) // 2
    closed = plain[:middle] + b'\xff\xd9'                       # tests/test_gpu_jpeg_decode.py's cut_and_closed: BAD_SCAN there
    call = CameraCall([good, closed, good], intervals=[0, 0, 2])
    assert call.decode() == 0, _lib.lib().kgdet_last_error()
    assert call.verdicts() == [NOT_EOI, BAD_SCAN, 0]
    assert np.array_equal(call.pictures()[2], dr.pil(good))
    old = CameraCall([closed], old=True)
    assert old.decode() == 0 and old.verdicts() == [BAD_SCAN]


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_every_refusal_writes_nothing():
    files = [cr.make('noise', 17, 33, 90, '422', ('blocks', 1)), cr.make('ramp', 33, 47, 50, '444'), cr.make('noise', 16, 17, 90, 'grey')]
    call = CameraCall(files)
    L = _lib.lib()
    changes = dict(negative_interval=dict(reserved=(0, -1)), wide_interval=dict(reserved=(1, 65536)), mode=dict(mode=(1, 4)),
                   negative_mode=dict(mode=(0, -1)), zero_height=dict(H=(0, 0)), wide=dict(W=(1, 8193)), short_scan=dict(scan_bytes=(0, 1)))
    for name, change in changes.items():
        jobs = call.make_jobs(**change)
        assert call.decode(jobs=jobs) == _lib.KGDET_E_SHAPE, name
        assert L.kgdet_jpeg_decode_camera_workspace_bytes(jobs, i32(3)) == 0, name
        call.nothing_written()
    overrides = dict(small=dict(ws_bytes=call.ws_bytes - 1), many=dict(n=33), no_jobs=dict(jobs=None),
                     misaligned=dict(ws=vp(call.ws.data_ptr() + 8), ws_bytes=call.ws_bytes - 8))
    for name, override in overrides.items():
        assert call.decode(**override) == _lib.KGDET_E_SHAPE, name
        assert L.kgdet_last_error()
        call.nothing_written()
    assert call.decode(jobs=call.make_jobs(reserved=(2, 65535))) == 0      # the largest interval is taken
    old = CameraCall([files[1]], old=True)                      # and the old entry point still refuses mode 3, whatever `reserved` says
    assert old.decode(jobs=old.make_jobs(mode=(0, 3))) == _lib.KGDET_E_SHAPE
    old.nothing_written()
    assert old.decode(jobs=old.make_jobs(reserved=(0, -5))) == 0 and old.verdicts() == [0]
    for got, data in zip(call.run(), files):                    # the same call object decodes when nothing is wrong
        assert np.array_equal(got, dr.pil(data))


# ---- the decoder object ---------------------------------------------------------------------------------------------------------
def test_the_decoder_object_with_the_switch():
    files = [cr.make('noise', 23, 31, 90, '422', ('rows', 1)), cr.make('ramp', 40, 56, 50, '420', ('blocks', 3)),
             dr.make('noise', 33, 47, 90, '444'), cr.make('noise', 9, 17, 100, '422')]
    decoder = jpeg.DeviceJpegDecoder(camera=True)
    images, status = decoder(files)
    assert status.cpu().tolist() == [0] * 4
    for data, img in zip(files, images):
        assert np.array_equal(img.cpu().numpy(), dr.pil(data))
    _, status = decoder([files[0], cr.broken(cr.make('noise', 40, 56, 90, '422', ('blocks', 2)))['swapped']])
    assert status.cpu().tolist() == [0, BAD_RESTART]
    with pytest.raises(ValueError, match='restart interval'):
        jpeg.DeviceJpegDecoder()(files[:1])
    for data in files:
        assert np.array_equal(jpeg.decode_jpeg(data, camera=True), dr.pil(data))
        assert np.array_equal(jpeg.decode_jpeg(data), dr.pil(data))                # (PIL without the switch: the same bits)
