"""Shared by tests/test_jpeg_decode_refs.py, tests/test_gpu_jpeg_decode.py and tests/test_gpu_loader_decode.py: the JPEG files the
decoder is tried on (made here with PIL from tests/jpeg_refs.py's generators, plus the committed demo image), PIL's picture of
each, a census of what falls on the Huffman kernel's subsequence boundaries, and a plain-Python run of the kernel's
self-synchronising scheme on top of ``jpeg.decode_span``.  Nothing here is committed data."""
import functools
import io

import numpy as np

from kgdet_amd import jpeg

from . import jpeg_refs

S = jpeg.DECODE_SUBSEQ_BITS
LANES = jpeg.DECODE_CHUNK_LANES


def uniform(H, W, seed):
    """white everywhere, the background of a shop photograph: a periodic stream (every MCU after the first codes the same 32
    bits with the standard tables) in which a parse that starts a few blocks off stays consistent and never meets the true one"""
    return np.full((H, W, 3), 255, dtype=np.uint8)


GENERATORS = dict(noise=jpeg_refs.noise, ramp=jpeg_refs.ramp, checker=jpeg_refs.checker, grey=jpeg_refs.grey, uniform=uniform)
KINDS = {'420': dict(subsampling=2), '444': dict(subsampling=0), 'grey': None,
         '420-opt': dict(subsampling=2, optimize=True), '444-opt': dict(subsampling=0, optimize=True), 'grey-opt': dict(optimize=True)}


def write_jpeg(img, quality, kind, **more):
    """the file PIL writes for a uint8 [H, W, 3] array; the 'grey' kinds write its luminance as a one-component file"""
    from PIL import Image
    im = Image.fromarray(img)
    kw = dict(KINDS[kind] or {})
    if kind.startswith('grey'):
        im = im.convert('L')
    kw.update(more)
    buf = io.BytesIO()
    im.save(buf, 'JPEG', quality=quality, **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def make(content, H, W, quality, kind, seed=3):
    return write_jpeg(GENERATORS[content](H, W, seed), quality, kind)


@functools.lru_cache(maxsize=None)
def demo_file():
    with open(jpeg_refs.DEMO_IMAGE, 'rb') as f:
        return f.read()


def pil(data):
    return jpeg.decode_pil(data)


# ---- the cases -------------------------------------------------------------------------------------------------------------
SIZES_72 = ((24, 40), (33, 47), (80, 96), (17, 16), (1, 1), (16, 17))
QUALITIES = (90, 50, 100, 5)
# the 72 files the definition was first held to PIL on: noise / ramp / checker, 4:2:0
CASES_72 = [(c, H, W, q, '420') for c in ('noise', 'ramp', 'checker') for (H, W) in SIZES_72 for q in QUALITIES]
# the same sizes as 4:4:4, one component and with optimised Huffman tables (contents rotate, each meets every kind and quality)
CASES_KINDS = [(('noise', 'ramp', 'checker')[(i + j + k) % 3], H, W, q, kind)
               for i, (H, W) in enumerate(SIZES_72) for j, q in enumerate(QUALITIES)
               for k, kind in enumerate(('444', 'grey', '420-opt', '444-opt', 'grey-opt'))]

GPU_SIZES = ((1, 1), (8, 8), (17, 16), (16, 17), (33, 47), (80, 96))
GPU_QUALITIES = (5, 50, 90, 100)
# the kernels' cases: every size x kind x quality, the content rotating so that each meets every kind and quality
GPU_CASES = [(('noise', 'ramp', 'checker')[(i + j + k) % 3], H, W, q, kind)
             for i, (H, W) in enumerate(GPU_SIZES) for j, q in enumerate(GPU_QUALITIES) for k, kind in enumerate(KINDS)]
# a stream of more than one chunk of the Huffman kernel (LANES subsequences of S bits), asserted where it is used
LONG_CASE = ('noise', 200, 216, 100, '444')
UNIFORM_CASES = [('uniform', 256, 256, 90, '420'), ('uniform', 624, 468, 90, '420'), ('uniform', 624, 468, 90, '420-opt')]
BAD_SIZE = (33, 47)


def case_name(case):
    return '%s-%dx%d-q%d-%s' % case


@functools.lru_cache(maxsize=None)
def restated(case):
    """``jpeg.decode_parts`` of a case's file, computed once and shared (do not modify)"""
    return jpeg.decode_parts(make(*case))


# ---- what falls on the subsequence boundaries --------------------------------------------------------------------------------
CENSUS_KEYS = ('code_straddles', 'magnitude_straddles', 'block_ends_on_boundary', 'zrl', 'block_over_two_boundaries')


def boundary_census(data, subseq_bits=S):
    """Counts, over the TRUE parse of a file (the instrumented ``jpeg.decode_span``), of what the boundaries k * subseq_bits cut:
    a Huffman code (the boundary strictly inside its bits), the magnitude bits of a symbol that began before the boundary (the
    boundary at their first bit or inside them), a block whose last bit is the last bit before a boundary, and a block that
    holds two boundaries or more (the lane between them neither begins nor ends it); and the ZRL symbols."""
    trace = []
    jpeg.decode_parts(data, trace)
    out = dict.fromkeys(CENSUS_KEYS, 0)
    block_start = 0
    for p, length, s, symbol, z, ends in trace:
        code_end, end = p + length, p + length + s
        if (code_end - 1) // subseq_bits > p // subseq_bits:
            out['code_straddles'] += 1
        if s and (end - 1) // subseq_bits > (code_end - 1) // subseq_bits:
            out['magnitude_straddles'] += 1
        if symbol == 0xF0:
            out['zrl'] += 1
        if ends:
            if end % subseq_bits == 0:
                out['block_ends_on_boundary'] += 1
            # boundaries strictly inside the block's bits [block_start, end): after its first bit and before its last
            if (end - 1) // subseq_bits - block_start // subseq_bits >= 2:
                out['block_over_two_boundaries'] += 1
            block_start = end
    return out


def true_states(ctx, subseq_bits=S):
    """the exit state and the completed blocks of every subsequence on the true parse"""
    nsub = -(-ctx.total_bits // subseq_bits)
    state, out = (0, 0, 0), []
    for i in range(nsub):
        state, done = _lane(ctx, state, i, subseq_bits)
        out.append((state, done))
    return out


def _lane(ctx, entry, i, subseq_bits, sink=None):
    """a lane of the Huffman kernel: the symbols that start in subsequence i; a state outside it passes through"""
    start, limit = i * subseq_bits, (i + 1) * subseq_bits
    if entry == jpeg.INVALID or not (start <= entry[0] < limit) or entry[0] >= ctx.total_bits:
        return entry, 0
    return jpeg.decode_span(ctx, entry, limit, sink)


def cold_run(data, subseq_bits=S):
    """the longest run of subsequences a cold start (the subsequence's first bit, slot 0, index 0) does not synchronise in: for
    every start i >= 1 the number of subsequences i, i + 1, ... whose exit still differs from the true one"""
    parts = jpeg.decode_parts(data)
    ctx = parts['context']
    true = true_states(ctx, subseq_bits)
    best = 0
    for i in range(1, len(true)):
        state, j = (i * subseq_bits, 0, 0), i
        while j < len(true):
            state, _ = _lane(ctx, state, j, subseq_bits)
            if state == true[j][0]:
                break
            j += 1
        best = max(best, j - i)
        if best >= len(true) - 1 - i:
            break
    return best


def fixpoint_decode(data, subseq_bits=S, lanes=LANES):
    """The Huffman kernel's scheme in plain Python -> (coefficients int64 [blocks, 64] natural order with the DC DIFFERENCES,
    rounds per chunk, final state, blocks): chunks of ``lanes`` subsequences, lane 0 entering true and the others cold,
    exit[i] -> entry[i + 1] until nothing changes (an INVALID exit hands nothing on: the next lane keeps its cold start), then
    the write pass from the true entries.  For files whose true parse is valid."""
    frame = jpeg.parse_header(data)
    ctx = jpeg.EntropyContext(frame, jpeg.unstuff(data, frame['scan_offset']))
    mw, mh, bpm = jpeg.frame_blocks(frame)
    nblocks = mw * mh * bpm
    zz = np.zeros((nblocks, 64), dtype=np.int64)
    nsub = -(-ctx.total_bits // subseq_bits)
    chunk_entry, blocks, rounds = (0, 0, 0), 0, []
    for base in range(0, nsub, lanes):
        nl = min(lanes, nsub - base)
        entry = [chunk_entry] + [((base + t) * subseq_bits, 0, 0) for t in range(1, nl)]
        need, exits, done = [True] * nl, [None] * nl, [0] * nl
        for r in range(nl + 1):
            for t in range(nl):
                if need[t]:
                    exits[t], done[t] = _lane(ctx, entry[t], base + t, subseq_bits)
            handed = [exits[t - 1] if exits[t - 1] != jpeg.INVALID else ((base + t) * subseq_bits, 0, 0) for t in range(1, nl)]
            need = [False] + [handed[t - 1] != entry[t] for t in range(1, nl)]
            entry = [entry[0]] + handed
            if not any(need):
                rounds.append(r + 1)
                break
        else:
            raise AssertionError('no fixpoint after %d rounds' % (nl + 1))
        for t in range(nl):
            first = blocks + sum(done[:t])

            def sink(block, place, value, first=first):
                assert first + block < nblocks
                zz[first + block, place] = value
            again = _lane(ctx, entry[t], base + t, subseq_bits, sink)
            assert again == (exits[t], done[t])
        chunk_entry, blocks = exits[nl - 1], blocks + sum(done)
    coef = np.zeros_like(zz)
    coef[:, jpeg.ZIGZAG] = zz
    return coef, rounds, chunk_entry, blocks


# ---- files the decoder must refuse ---------------------------------------------------------------------------------------------
def insert_segments(data, segments, at_marker=0xDB):
    """``data`` with the raw ``segments`` (bytes) put in front of its first ``at_marker`` segment"""
    k = data.find(bytes([0xFF, at_marker]))
    assert k > 0
    return data[:k] + b''.join(segments) + data[k:]


def merge_tables(data, marker):
    """``data`` with all its ``DQT`` (0xDB) or ``DHT`` (0xC4) segments merged into ONE segment that holds every table"""
    at, out, bodies, where = 2, bytearray(data[:2]), [], None
    while True:
        assert data[at] == 0xFF
        m, n = data[at + 1], data[at + 2] << 8 | data[at + 3]
        if m == marker:
            bodies.append(data[at + 4:at + 2 + n])
            if where is None:
                where = len(out)
        else:
            if m == 0xDA:
                break
            out += data[at:at + 2 + n]
        at += 2 + n
    body = b''.join(bodies)
    merged = bytes([0xFF, marker, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + body
    return bytes(out[:where]) + merged + bytes(out[where:]) + data[at:]


def scan_start(data):
    frame = jpeg.parse_header(data)
    assert not isinstance(frame, str), frame
    return frame['scan_offset']
