"""``kgdet_jpeg_decode`` (csrc/jpeg_decode.hip) through the C ABI.

The bar is EQUALITY of every byte of the picture with ``jpeg.decode_restatement`` (held to PIL's decoder on the CPU by
tests/test_jpeg_decode_refs.py) and, for the larger files, with PIL itself.  Output and workspace are pre-filled with 0xA5 and
sit between 64-byte canaries; scans, table blocks and pictures lie at odd offsets with gaps between them: every byte of a
picture must be written, nothing beside it, and the source must come back unchanged."""
import ctypes

import numpy as np
import pytest
import torch

from kgdet_amd import _lib, jpeg
from tests import jpeg_decode_refs as dr

pytestmark = pytest.mark.gpu
i32, i64, vp, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
FILL, CANARY, PAD = 0xA5, 0x5C, 64


class Call(object):
    """one ``kgdet_jpeg_decode`` of ``files``: scan i (from the first entropy byte to the file's end) and its table block lie at
    odd offsets of the source buffer, picture i at an odd offset of the output buffer with a gap of 5 bytes behind it"""

    def __init__(self, files):
        self.files, self.n = files, len(files)
        self.frames = [jpeg.parse_header(f) for f in files]
        assert not any(isinstance(f, str) for f in self.frames), self.frames
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
        self.ws_bytes = _lib.lib().kgdet_jpeg_decode_workspace_bytes(self.jobs, i32(self.n)) if self.n else 256
        assert self.ws_bytes > 0
        self.ws_all = torch.full((self.ws_bytes + 2 * PAD,), FILL, dtype=torch.uint8, device='cuda')
        self.ws_all[:PAD] = CANARY
        self.ws_all[PAD + self.ws_bytes:] = CANARY
        self.ws = self.ws_all[PAD:PAD + self.ws_bytes]
        self.status = torch.full((self.n + 2,), -7, dtype=torch.int32, device='cuda')

    def make_jobs(self, **change):
        """the job table; ``change``: {field: (image, value)}"""
        rows = [dict(scan_offset=so, scan_bytes=sb, tables_offset=to, dst_offset=at, H=f['H'], W=f['W'], mode=f['mode'], reserved=0)
                for (so, sb, to), at, f in zip(self.places, self.out_at, self.frames)]
        for field, (i, value) in change.items():
            rows[i][field] = value
        return (_lib.JpegDecodeJob * max(self.n, 1))(*[_lib.JpegDecodeJob(**r) for r in rows])

    def decode(self, **override):
        a = dict(src=_lib.ptr(self.src), src_bytes=self.src.numel(), jobs=self.jobs, n=self.n, ws=_lib.ptr(self.ws),
                 ws_bytes=self.ws_bytes, out=_lib.ptr(self.out), out_bytes=self.out.numel(), status=vp(self.status.data_ptr() + 4))
        a.update(override)
        rc = _lib.lib().kgdet_jpeg_decode(a['src'], i64(a['src_bytes']), a['jobs'], i32(a['n']), a['ws'], sz(a['ws_bytes']), a['out'],
                                          i64(a['out_bytes']), a['status'], _lib.current_stream())
        torch.cuda.synchronize()
        return rc

    def verdicts(self):
        host = self.status.cpu().numpy()
        assert host[0] == -7 and host[-1] == -7, 'written beside the status'
        return host[1:-1].tolist()

    def pictures(self):
        """the pictures as written (the region of an image whose status is not 0 may hold anything); asserts the canaries, every
        byte outside the pictures, the workspace's canaries and the source"""
        host = self.out.cpu().numpy()
        assert (host[:PAD] == CANARY).all() and (host[-PAD:] == CANARY).all(), 'a canary of the output was overwritten'
        mask = np.ones(host.size, dtype=bool)
        mask[:PAD] = mask[-PAD:] = False
        got = []
        for at, f in zip(self.out_at, self.frames):
            size = 3 * f['H'] * f['W']
            mask[at:at + size] = False
            got.append(host[at:at + size].reshape(f['H'], f['W'], 3))
        assert (host[mask] == FILL).all(), 'bytes beside the pictures were written'
        ws = self.ws_all.cpu().numpy()
        assert (ws[:PAD] == CANARY).all() and (ws[PAD + self.ws_bytes:] == CANARY).all(), 'a canary of the workspace was overwritten'
        assert np.array_equal(self.src.cpu().numpy(), self.src_host), 'the source was written'
        return got

    def nothing_written(self):
        host = self.out.cpu().numpy()
        assert (host[:PAD] == CANARY).all() and (host[-PAD:] == CANARY).all() and (host[PAD:-PAD] == FILL).all()
        ws = self.ws_all.cpu().numpy()
        assert (ws[:PAD] == CANARY).all() and (ws[PAD + self.ws_bytes:] == CANARY).all() and (ws[PAD:PAD + self.ws_bytes] == FILL).all()
        assert (self.status.cpu().numpy() == -7).all()
        assert np.array_equal(self.src.cpu().numpy(), self.src_host)

    def rounds(self):
        """the fixpoint's rounds per image, the second uint32 [32] of the workspace"""
        return self.ws[128:128 + 4 * self.n].view(torch.int32).cpu().tolist()

    def run(self):
        assert self.decode() == 0, _lib.lib().kgdet_last_error()
        assert self.verdicts() == [0] * self.n
        return self.pictures()


def decoded(files):
    out = []
    for g in range(0, len(files), jpeg.DECODE_MAX_IMAGES):
        out.extend(Call(files[g:g + jpeg.DECODE_MAX_IMAGES]).run())
    return out


def test_every_size_kind_and_quality_equals_the_restatement_and_pil():
    files = [dr.make(*case) for case in dr.GPU_CASES]
    assert {(c[1], c[2]) for c in dr.GPU_CASES} == {(1, 1), (8, 8), (17, 16), (16, 17), (33, 47), (80, 96)}
    assert {c[3] for c in dr.GPU_CASES} == {5, 50, 90, 100} and {c[4] for c in dr.GPU_CASES} == set(dr.KINDS)
    for case, data, got in zip(dr.GPU_CASES, files, decoded(files)):
        assert np.array_equal(got, dr.restated(case)['image']), dr.case_name(case)
        assert np.array_equal(got, dr.pil(data)), dr.case_name(case)


def test_a_stream_of_more_than_one_chunk():
    data = dr.make(*dr.LONG_CASE)
    frame = jpeg.parse_header(data)
    stream_bits = 8 * len(jpeg.unstuff(data, frame['scan_offset']))
    assert stream_bits > 2 * jpeg.DECODE_SUBSEQ_BITS * jpeg.DECODE_CHUNK_LANES      # three chunks of the workgroup
    got, = Call([data]).run()
    assert np.array_equal(got, dr.pil(data))


def test_uniform_pictures_take_as_many_rounds_as_subsequences_and_decode():
    files = [dr.make(*case) for case in dr.UNIFORM_CASES]
    call = Call(files)
    for case, data, got in zip(dr.UNIFORM_CASES, files, call.run()):
        assert np.array_equal(got, dr.pil(data)), dr.case_name(case)
    assert np.array_equal(call.pictures()[0], dr.restated(dr.UNIFORM_CASES[0])['image'])
    # the shifted parses never meet the true one: the true state walks through the stream a lane per round
    expected = [max(dr.fixpoint_decode(data)[1]) for data in files]
    assert call.rounds() == expected and min(expected) >= 17, (call.rounds(), expected)


def test_the_demo_image_equals_pil_and_the_restatement():
    data = dr.demo_file()
    call = Call([data])
    got, = call.run()
    assert got.shape == (624, 468, 3)
    assert np.array_equal(got, dr.pil(data))
    assert np.array_equal(got, jpeg.decode_restatement(data))
    assert call.rounds() == [max(dr.fixpoint_decode(data)[1])]


def mixed_batch():
    files = [dr.make(*case) for case in dr.GPU_CASES[5::5][:28]]
    return files + [dr.demo_file(), dr.make(*dr.UNIFORM_CASES[0]), dr.make('noise', 80, 96, 100, '444'), dr.make('ramp', 1, 1, 90, 'grey')]


def test_a_batch_of_32_equals_32_calls_of_one():
    files = mixed_batch()
    assert len(files) == jpeg.DECODE_MAX_IMAGES == 32
    assert len({jpeg.parse_header(f)['mode'] for f in files}) == 3
    together = Call(files).run()
    for k, (data, got) in enumerate(zip(files, together)):
        alone, = Call([data]).run()
        assert np.array_equal(got, alone), k
        assert np.array_equal(got, dr.pil(data)), k


def test_no_images_is_a_no_op():
    call = Call([dr.make('noise', 8, 8, 90, '420')])
    assert call.decode(n=0) == 0
    call.nothing_written()
    assert call.decode(n=0, src=vp(0), jobs=None, ws=vp(0), out=vp(0), status=vp(0)) == 0
    assert _lib.lib().kgdet_jpeg_decode_workspace_bytes(None, i32(0)) > 0


def test_every_refusal_writes_nothing():
    files = [dr.make('noise', 17, 16, 90, '420'), dr.make('ramp', 33, 47, 50, '444'), dr.make('checker', 16, 17, 90, 'grey')]
    call = Call(files)
    L = _lib.lib()
    size1 = 3 * 33 * 47
    changes = dict(
        zero_height=dict(H=(0, 0)), wide=dict(W=(1, 8193)), negative_width=dict(W=(2, -1)), mode=dict(mode=(1, 3)),
        negative_mode=dict(mode=(0, -1)), short_scan=dict(scan_bytes=(0, 1)), huge_scan=dict(scan_bytes=(0, (1 << 28) + 1)),
        scan_before=dict(scan_offset=(1, -1)), scan_behind=dict(scan_offset=(2, call.src.numel() - call.places[2][1] + 1)),
        tables_before=dict(tables_offset=(0, -1)), tables_behind=dict(tables_offset=(1, call.src.numel() - jpeg.DECODE_TABLE_BYTES + 1)),
        picture_before=dict(dst_offset=(0, -1)), picture_behind=dict(dst_offset=(1, call.out.numel() - size1 + 1)),
        pictures_overlap=dict(dst_offset=(2, call.out_at[1] + size1 - 1)))
    for name, change in changes.items():
        jobs = call.make_jobs(**change)
        assert call.decode(jobs=jobs) == _lib.KGDET_E_SHAPE, name
        assert L.kgdet_jpeg_decode_workspace_bytes(jobs, i32(3)) == 0 or name.split('_')[0] in ('scan', 'tables', 'picture', 'pictures'), name
        call.nothing_written()
    a = call.src.data_ptr()
    overrides = dict(
        many=dict(n=33), negative_n=dict(n=-1), no_source=dict(src=vp(0)), no_jobs=dict(jobs=None), no_workspace=dict(ws=vp(0)),
        no_output=dict(out=vp(0)), no_status=dict(status=vp(0)), negative_source=dict(src_bytes=-1), negative_output=dict(out_bytes=-1),
        misaligned=dict(ws=vp(call.ws.data_ptr() + 8), ws_bytes=call.ws_bytes - 8), small=dict(ws_bytes=call.ws_bytes - 1),
        output_in_source=dict(out=vp(a), out_bytes=min(call.src.numel(), call.out.numel())),
        output_in_workspace=dict(out=vp(call.ws.data_ptr() + 256)),
        status_in_output=dict(status=vp(call.out.data_ptr() + PAD)), status_in_workspace=dict(status=vp(call.ws.data_ptr() + 16)),
        status_in_source=dict(status=vp(a + 4)))
    for name, override in overrides.items():
        if name == 'output_in_workspace':
            assert call.ws_bytes >= 256 + call.out.numel()
        assert call.decode(**override) == _lib.KGDET_E_SHAPE, name
        assert L.kgdet_last_error()
        call.nothing_written()
    assert L.kgdet_jpeg_decode_workspace_bytes(call.jobs, i32(33)) == 0 and L.kgdet_jpeg_decode_workspace_bytes(None, i32(1)) == 0
    for got, data in zip(call.run(), files):                    # and the same call object decodes when nothing is wrong
        assert np.array_equal(got, dr.pil(data))


def bad_files():
    """files of 33 x 47 a correct decoder refuses cleanly -> {name: bytes}"""
    H, W = dr.BAD_SIZE
    good = dr.make('noise', H, W, 90, '420')
    start = dr.scan_start(good)
    middle = start + (len(good) - start) // 2
    rng = np.random.default_rng(11)
    tail = bytes(int(v) for v in rng.integers(0, 255, len(good) - 2 - middle))          # (no 0xFF: no marker among them)
    other = dr.make('ramp', H, W, 90, '444')
    return dict(cut_in_the_middle=good[:middle], cut_and_closed=good[:middle] + b'\xff\xd9', random_tail=good[:middle] + tail + b'\xff\xd9',
                without_eoi=good[:-2], restart_marker_ends_it=good[:middle] + b'\xff\xd0' + good[middle:],
                too_many_blocks=good[:start] + other[dr.scan_start(other):], a_last_byte_of_ff=good[:-2] + b'\xff')


@pytest.mark.parametrize('name', sorted(bad_files()))
def test_a_bad_stream_gets_a_status_and_touches_nothing_else(name):
    H, W = dr.BAD_SIZE
    bad = bad_files()[name]
    neighbours = [dr.make('checker', H, W, 50, '420'), dr.make('ramp', H, W, 100, '444-opt')]
    call = Call([neighbours[0], bad, neighbours[1]])
    assert call.decode() == 0, _lib.lib().kgdet_last_error()
    status = call.verdicts()
    assert status[0] == 0 and status[2] == 0 and status[1] != 0, status
    expected = dict(cut_in_the_middle=1, without_eoi=1, a_last_byte_of_ff=1, restart_marker_ends_it=2, cut_and_closed=3, too_many_blocks=3)
    assert name not in expected or status[1] == expected[name], status
    got = call.pictures()
    assert np.array_equal(got[0], dr.pil(neighbours[0])) and np.array_equal(got[2], dr.pil(neighbours[1]))
    with pytest.raises(ValueError):
        jpeg.decode_restatement(bad)


def test_the_decoder_object_and_decode_jpeg():
    files = mixed_batch() + [dr.make('noise', 33, 47, 50, '420-opt')]            # 33 files: two groups
    decoder = jpeg.DeviceJpegDecoder()
    images, status = decoder(files)
    assert status.dtype == torch.int32 and status.cpu().tolist() == [0] * 33
    store = images[0].untyped_storage().data_ptr()
    for data, img in zip(files, images):
        assert img.is_cuda and img.dtype == torch.uint8 and img.is_contiguous() and img.untyped_storage().data_ptr() == store
        assert np.array_equal(img.cpu().numpy(), dr.pil(data))
    again, _ = decoder(files[:3])                                # the staging buffer and the workspace are reused
    assert all(np.array_equal(a.cpu().numpy(), dr.pil(d)) for a, d in zip(again, files))
    with pytest.raises(ValueError, match='progressive'):
        decoder([dr.write_jpeg(dr.GENERATORS['noise'](16, 16, 0), 90, '420', progressive=True)])
    bad = bad_files()['cut_and_closed']
    _, status = decoder([files[0], bad])
    assert status.cpu().tolist()[0] == 0 and status.cpu().tolist()[1] != 0
    for data in (files[0], dr.demo_file(), dr.write_jpeg(dr.GENERATORS['noise'](16, 16, 0), 90, '420', progressive=True)):
        assert np.array_equal(jpeg.decode_jpeg(data), dr.pil(data))


def test_a_call_cut_short_says_so_and_the_decoder_serves_any_stream():
    files = [dr.make('noise', 80, 96, 90, '420'), dr.make('ramp', 33, 47, 50, '444')]
    frames = [jpeg.parse_header(f) for f in files]
    total, places = jpeg.pack_files(files, frames)
    host = np.zeros(total, dtype=np.uint8)
    jpeg.pack_files(files, frames, host)
    src = torch.from_numpy(host).cuda()
    jobs = [(so, sb, to, f['H'], f['W'], f['mode']) for (so, sb, to), f in zip(places, frames)]
    decoder = jpeg.DeviceJpegDecoder()
    for stages in (1, 2, 3):
        _, status = decoder.decode(src, jobs, stages=stages)
        assert status.cpu().tolist() == [-1, -1], stages                # KGDET_JPEG_DECODE_STOPPED: no picture, and no status 0
    with pytest.raises(RuntimeError, match='stages'):
        decoder.decode(src, jobs, stages=5)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    kept = []
    for k in range(6):                                                  # one workspace, two streams in turn, nothing waited for
        with torch.cuda.stream(side if k % 2 else torch.cuda.current_stream()):
            kept.append(decoder.decode(src, jobs[::-1] if k % 3 == 0 else jobs))
    torch.cuda.synchronize()
    for k, (images, status) in enumerate(kept):
        want = files[::-1] if k % 3 == 0 else files
        assert status.cpu().tolist() == [0, 0]
        assert all(np.array_equal(img.cpu().numpy(), dr.pil(data)) for img, data in zip(images, want)), k
