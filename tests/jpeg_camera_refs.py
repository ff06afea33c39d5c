"""Shared by tests/test_jpeg_camera_refs.py, tests/test_gpu_jpeg_camera.py and tests/test_gpu_loader_camera.py: the files of the
``camera`` switch of the JPEG decoder -- 4:2:2 sampling and restart intervals -- made here with PIL (``subsampling='4:2:2'``,
``restart_marker_blocks`` / ``restart_marker_rows``) from tests/jpeg_decode_refs.py's generators, and the ways a restart file is
broken.  Nothing here is committed data."""
import functools
import io

from kgdet_amd import jpeg

from . import jpeg_decode_refs as dr

SUBSAMPLING = {'420': '4:2:0', '422': '4:2:2', '444': '4:4:4', 'grey': None}
# (PIL's keyword, its value): no restart markers, an interval of 1 and of 3 MCUs, of one and of two MCU rows
RESTARTS = (None, ('blocks', 1), ('blocks', 3), ('rows', 1), ('rows', 2))
SIZES = ((1, 1), (8, 16), (9, 17), (23, 31), (40, 56), (33, 130), (70, 49))
# the grid the definition is held to PIL on: 560 files, and 560 more with optimised Huffman tables at the extreme qualities
GRID = [(content, H, W, q, kind, restart, False) for kind in SUBSAMPLING for content in ('noise', 'ramp') for (H, W) in SIZES
        for q in (30, 90) for restart in RESTARTS]
GRID_OPT = [(content, H, W, q, kind, restart, True) for kind in SUBSAMPLING for content in ('noise', 'ramp') for (H, W) in SIZES
            for q in (5, 100) for restart in RESTARTS]


def write_jpeg(img, quality, kind, restart=None, optimize=False):
    """the file PIL writes for a uint8 [H, W, 3] array; ``kind`` a key of ``SUBSAMPLING`` ('grey': its luminance as a
    one-component file); ``restart``: None or ('blocks' | 'rows', n)"""
    from PIL import Image
    im = Image.fromarray(img)
    kw = dict(quality=quality, optimize=optimize)
    if kind == 'grey':
        im = im.convert('L')
    else:
        kw['subsampling'] = SUBSAMPLING[kind]
    if restart is not None:
        kw['restart_marker_' + restart[0]] = restart[1]
    buf = io.BytesIO()
    im.save(buf, 'JPEG', **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def make(content, H, W, quality, kind, restart=None, optimize=False, seed=3):
    return write_jpeg(dr.GENERATORS[content](H, W, seed), quality, kind, restart, optimize)


def case_name(case):
    return '%s-%dx%d-q%d-%s-%s-%s' % (case[:5] + ('none' if case[5] is None else '%s%d' % case[5], 'opt' if case[6] else 'std'))


@functools.lru_cache(maxsize=None)
def restated(case):
    """``jpeg.decode_restatement(camera=True)`` of a case's file, computed once and shared (do not modify)"""
    return jpeg.decode_restatement(make(*case), camera=True)


def frame_of(data):
    frame = jpeg.parse_header(data, camera=True)
    assert not isinstance(frame, str), frame
    return frame


def markers(data):
    """[(offset of the 0xFF, m)] of the restart markers in the scan of a file, in file order"""
    at, out = frame_of(data)['scan_offset'], []
    while True:
        at = data.index(b'\xff', at)
        nxt = data[at + 1]
        if 0xD0 <= nxt <= 0xD7:
            out.append((at, nxt - 0xD0))
        elif nxt != 0:
            assert nxt == 0xD9, 'marker %02X in the scan' % nxt
            return out
        at += 2


def broken(data):
    """a restart file (at least four markers) broken in the ways the decoder must name -> {name: bytes}"""
    data, found = bytearray(data), markers(data)
    assert len(found) >= 4 and [m for _, m in found[:4]] == [0, 1, 2, 3]
    (a, _), (b, _), (c, _) = found[0], found[1], found[2]

    def patched(changes):
        out = bytearray(data)
        for at, m in changes:
            out[at + 1] = 0xD0 + m
        return bytes(out)
    cut = (b + c) // 2                                       # inside interval 2: its tail is dropped
    while data[cut - 1] == 0xFF:                             # (never between an 0xFF and its stuffed 0x00)
        cut -= 1
    assert cut > b + 2
    return dict(swapped=patched([(a, 1), (b, 0)]), missing=bytes(data[:b] + data[b + 2:]),
                surplus=bytes(data[:b] + data[b:b + 2] + data[b:]), out_of_order=patched([(b, 0)]),
                cut_short=bytes(data[:cut] + data[c:]))
