"""Shared by tests/test_jpeg_refs.py, tests/test_gpu_jpeg.py and tests/test_gpu_show_jpeg.py: a float64 reference of the
coefficient stage of ``jpeg.jpeg_restatement``, a parser of the entropy layer written for these tests, and the case list.
Nothing here is committed data; the one picture read is tests/golden/demo_images/079952.jpg."""
import functools
import os

import numpy as np

from kgdet_amd import jpeg

DEMO_IMAGE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'demo_images', '079952.jpg')


# ---- the float64 reference of the coefficient stage ----------------------------------------------------------------------
def exact_ratios(image, quality):
    """coefficient / table entry BEFORE rounding, everything exact in float64: the JFIF matrix, the same edge rule, the exact
    mean of each 2 x 2, an exact DCT-II -> (Y [2 mh, 2 mw, 8, 8], Cb, Cr [mh, mw, 8, 8])"""
    H, W = image.shape[:2]
    mh, mw = (H + 15) // 16, (W + 15) // 16
    px = np.pad(image.astype(np.float64), ((0, 16 * mh - H), (0, 16 * mw - W), (0, 0)), mode='edge')
    R, G, B = px[..., 0], px[..., 1], px[..., 2]
    Y = 0.299 * R + 0.587 * G + 0.114 * B
    Cb = -0.168736 * R - 0.331264 * G + 0.5 * B + 128.0
    Cr = 0.5 * R - 0.418688 * G - 0.081312 * B + 128.0
    Cb, Cr = (c.reshape(8 * mh, 2, 8 * mw, 2).mean(axis=(1, 3)) for c in (Cb, Cr))
    x = np.arange(8)
    A = np.cos((2 * x[None, :] + 1) * x[:, None] * np.pi / 16) * 0.5
    A[0] = np.sqrt(0.125)
    Q = jpeg.quant_tables(quality).astype(np.float64)
    out = []
    for plane, q in ((Y, Q[0]), (Cb, Q[1]), (Cr, Q[1])):
        a, b = plane.shape[0] // 8, plane.shape[1] // 8
        X = (plane - 128.0).reshape(a, 8, b, 8).transpose(0, 2, 1, 3)
        out.append(np.einsum('vy,abyx,ux->abvu', A, X, A) / q.reshape(8, 8))
    return tuple(out)


def round_half_away(v):
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def exact_idct(levels, q):
    """[a, b, 8, 8] quantised levels and a table [64] -> the exact inverse DCT of the dequantised blocks + 128, float64 [8a, 8b]"""
    x = np.arange(8)
    A = np.cos((2 * x[None, :] + 1) * x[:, None] * np.pi / 16) * 0.5
    A[0] = np.sqrt(0.125)
    F = levels.astype(np.float64) * q.reshape(8, 8).astype(np.float64)
    X = np.einsum('vy,abvu,ux->abyx', A, F, A) + 128.0
    a, b = levels.shape[:2]
    return X.transpose(0, 2, 1, 3).reshape(8 * a, 8 * b)


# ---- the parser ------------------------------------------------------------------------------------------------------------
def _decode_table(bits, vals):
    """(symbol, length) by the next 16 bits of the stream: int32 [65536, 2], length 0 where no code matches"""
    lut = np.zeros((65536, 2), dtype=np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            lo = code << (16 - length)
            lut[lo:lo + (1 << (16 - length))] = (vals[k], length)
            code, k = code + 1, k + 1
        code <<= 1
    assert k == len(vals)
    return lut


def parse(data):
    """Walk the markers of a baseline JFIF file, check every segment length, un-stuff the scan, Huffman-decode it with the tables
    found IN THE FILE -> dict(markers, app0, qt {id: [64] natural}, sof=(precision, H, W, [(id, h, v, tq)]), sos=[(id, td, ta)],
    spectral=(ss, se, ahal), blocks=(Y, Cb, Cr) in ``jpeg.quantized_blocks``' layout, bits = the stream's bits before the padding,
    stream = the un-stuffed scan bytes)"""
    assert data[:2] == b'\xff\xd8', 'no SOI'
    out = dict(markers=[0xD8], qt={}, huff={})
    at = 2
    while True:
        assert data[at] == 0xFF, 'no marker at %d' % at
        marker = data[at + 1]
        n = data[at + 2] << 8 | data[at + 3]
        body = data[at + 4:at + 2 + n]
        assert len(body) == n - 2, 'segment %02X runs past the file' % marker
        out['markers'].append(marker)
        if marker == 0xE0:
            assert n == 16
            out['app0'] = bytes(body)
        elif marker == 0xDB:
            assert n == 67 and body[0] >> 4 == 0, 'one 8-bit table per DQT'
            table = np.zeros(64, dtype=np.int64)
            table[jpeg.ZIGZAG] = list(body[1:])
            out['qt'][body[0] & 15] = table
        elif marker == 0xC0:
            assert n == 8 + 3 * body[5]
            comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(body[5])]
            out['sof'] = (body[0], body[1] << 8 | body[2], body[3] << 8 | body[4], comps)
        elif marker == 0xC4:
            bits = list(body[1:17])
            assert n == 19 + sum(bits), 'one table per DHT'
            out['huff'][body[0]] = _decode_table(bits, list(body[17:]))
        elif marker == 0xDA:
            assert n == 6 + 2 * body[0]
            out['sos'] = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(body[0])]
            out['spectral'] = tuple(body[1 + 2 * body[0]:])
            at += 2 + n
            break
        else:
            raise AssertionError('unexpected marker %02X' % marker)
        at += 2 + n
    assert data[-2:] == b'\xff\xd9', 'no EOI at the end'
    out['markers'].append(0xD9)
    scan = data[at:-2]
    k = scan.find(b'\xff')
    while k >= 0:
        assert k + 1 < len(scan) and scan[k + 1] == 0, 'an un-stuffed 0xFF in the data at %d' % (at + k)
        k = scan.find(b'\xff', k + 2)
    stream = scan.replace(b'\xff\x00', b'\xff')
    out['stream'] = stream
    bit = np.unpackbits(np.frombuffer(stream + b'\xff\xff', dtype=np.uint8)).astype(np.int64)
    nbits = 8 * len(stream)
    window = np.zeros(nbits + 1, dtype=np.int64)
    for j in range(16):
        window += bit[j:j + nbits + 1] << (15 - j)
    window = window.tolist()
    _, H, W, comps = out['sof']
    assert [c[1:3] for c in comps] == [(2, 2), (1, 1), (1, 1)], 'the parser reads 4:2:0 only'
    mh, mw = (H + 15) // 16, (W + 15) // 16
    planes = [np.zeros((2 * mh, 2 * mw, 64), dtype=np.int64), np.zeros((mh, mw, 64), dtype=np.int64),
              np.zeros((mh, mw, 64), dtype=np.int64)]
    tables = [(out['huff'][td].tolist(), out['huff'][0x10 | ta].tolist()) for _, td, ta in out['sos']]
    pos, pred = 0, [0, 0, 0]

    def receive(s):
        nonlocal pos
        if s == 0:
            return 0
        v = window[pos] >> (16 - s)
        pos += s
        return v if v >> (s - 1) else v - (1 << s) + 1

    for my in range(mh):
        for mx in range(mw):
            for comp, by, bx in ((0, 2 * my, 2 * mx), (0, 2 * my, 2 * mx + 1), (0, 2 * my + 1, 2 * mx), (0, 2 * my + 1, 2 * mx + 1),
                                 (1, my, mx), (2, my, mx)):
                dc, ac = tables[comp]
                s, length = dc[window[pos]]
                assert length and s <= 11, 'no DC code at bit %d' % pos
                pos += length
                pred[comp] += receive(s)
                blk = planes[comp][by, bx]
                blk[0] = pred[comp]
                k = 1
                while k < 64:
                    rs, length = ac[window[pos]]
                    assert length, 'no AC code at bit %d' % pos
                    pos += length
                    run, s = rs >> 4, rs & 15
                    if s == 0:
                        if run != 15:
                            assert run == 0
                            break
                        k += 16
                        assert k < 64, 'a ZRL past the block'
                        continue
                    k += run
                    assert k < 64 and s <= 10
                    blk[k] = receive(s)
                    k += 1
                assert pos <= nbits
    assert nbits - 8 < pos <= nbits, 'the scan ends %d bits before the data does' % (nbits - pos)
    assert all(bit[pos:nbits] == 1), 'the padding is not 1-bits'
    out['bits'] = pos
    natural = []
    for p in planes:
        nat = np.zeros_like(p)
        nat[..., jpeg.ZIGZAG] = p
        natural.append(nat.reshape(p.shape[0], p.shape[1], 8, 8))
    out['blocks'] = tuple(natural)
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------
def grey(H, W, seed):
    return np.full((H, W, 3), 128, dtype=np.uint8)


def noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


RAMP_TERMS = (63, 40, 17, 35, 58, 62)       # zigzag places of the isolated term, by (block row + 2 block column) mod 6


def ramp(H, W, seed):
    """a smooth grey ramp plus, per 8 x 8 block, one basis function far up the zigzag: zero runs of 16 and more in front of it,
    at place 63 a run that ends the block (no EOB), elsewhere ZRLs followed by EOB"""
    y, x = np.mgrid[0:H, 0:W]
    place = jpeg.ZIGZAG[np.array(RAMP_TERMS)[((y // 8) + 2 * (x // 8)) % 6]]
    v, u = place // 8, place % 8
    term = np.cos((2 * (y % 8) + 1) * v * np.pi / 16) * np.cos((2 * (x % 8) + 1) * u * np.pi / 16)
    value = 90.0 + 0.4 * x + 0.25 * y + 36.0 * term
    return np.repeat(np.clip(np.rint(value), 0, 255).astype(np.uint8)[..., None], 3, axis=2)


def checker(H, W, seed):
    """saturated black / white: a one-pixel checkerboard in the upper half (the largest AC magnitudes), 8 x 8 blocks of black
    and white below it (the largest DC differences: size category 11 at quality 100)"""
    y, x = np.mgrid[0:H, 0:W]
    fine, coarse = (x + y) % 2, ((x // 8) + (y // 8)) % 2
    value = np.where(y < (H + 1) // 2, fine, coarse) * 255
    return np.repeat(value.astype(np.uint8)[..., None], 3, axis=2)


def demo(H, W, seed):
    from PIL import Image
    with Image.open(DEMO_IMAGE) as im:
        img = np.array(im.convert('RGB'))
    assert img.shape == (H, W, 3)
    return img


# (name, content, H, W, seed); the sizes: 1 x 1, one block, one MCU, replication both ways with partial MCUs, several MCU rows
MULTI_RANGE = 'noise-112x96'                # its stream spans three of the pack kernel's ranges, on seven MCU rows
PAD_FF = 'noise-16x16'                      # at quality 100 its last byte is 0xFF once padded (seed found by search)
CASES = [
    ('grey-1x1', grey, 1, 1, 0), ('grey-16x16', grey, 16, 16, 0), ('grey-24x40', grey, 24, 40, 0),
    ('noise-1x1', noise, 1, 1, 5), ('noise-8x8', noise, 8, 8, 1), ('noise-16x16', noise, 16, 16, 33), ('noise-9x17', noise, 9, 17, 2),
    ('noise-17x9', noise, 17, 9, 3), ('noise-80x96', noise, 80, 96, 4), ('noise-112x96', noise, 112, 96, 6),
    ('ramp-24x40', ramp, 24, 40, 0), ('ramp-80x96', ramp, 80, 96, 0), ('ramp-17x9', ramp, 17, 9, 0),
    ('checker-16x16', checker, 16, 16, 0), ('checker-9x17', checker, 9, 17, 0), ('checker-24x40', checker, 24, 40, 0),
    ('demo-624x468', demo, 624, 468, 0),
]
MORE_QUALITIES = {'noise-16x16': (1, 50, 100), 'checker-24x40': (1, 50, 100)}
RUNS = [(c[0], q) for c in CASES for q in (90,) + MORE_QUALITIES.get(c[0], ())]
BY_NAME = {c[0]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def image(name):
    _, make, H, W, seed = BY_NAME[name]
    img = make(H, W, seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def restated(name, quality):
    """``jpeg.jpeg_parts`` of a case, computed once and shared by every test that needs it (do not modify)"""
    return jpeg.jpeg_parts(image(name), quality)


def check_case_list():
    """what the list has to cover, asserted from the restatement's own results"""
    residues, padded_ff = set(), []
    for name, q in RUNS:
        parts = restated(name, q)
        residues.add(parts['bits'] % 8)
        if parts['bits'] % 8 and parts['stream'][-1] == 0xFF:
            padded_ff.append((name, q))
    assert residues == set(range(8)), 'bit counts before padding take the residues %s mod 8' % sorted(residues)
    assert (PAD_FF, 100) in padded_ff, padded_ff
    multi = restated(MULTI_RANGE, 90)
    assert len(multi['stream']) > 2 * jpeg.RANGE_BYTES and BY_NAME[MULTI_RANGE][2] > 16
    assert restated('noise-80x96', 90)['stream'].count(b'\xff') >= 8
    for name in ('grey-1x1', 'grey-16x16', 'grey-24x40'):        # every block EOB, every DC difference 0
        parts = restated(name, 90)
        assert all((b == 0).all() for b in parts['blocks'])
        assert parts['bits'] == (4 * (2 + 4) + 2 * (2 + 2)) * parts['blocks'][1].shape[0] * parts['blocks'][1].shape[1]
    zz = restated('ramp-80x96', 90)['blocks'][0].reshape(-1, 64)[:, jpeg.ZIGZAG]
    ends = [(np.nonzero(b[1:])[0] + 1) for b in zz]
    assert any(len(e) >= 1 and e[-1] == 63 and (len(e) == 1 or e[-1] - e[-2] > 16) for e in ends), 'no long run up to place 63'
    assert any(len(e) >= 2 and e[-1] < 63 and e[-1] - e[-2] > 16 for e in ends), 'no ZRL in a block that ends in EOB'
    assert any(len(e) >= 2 and e[-1] - e[-2] > 32 for e in ends), 'no run of two ZRLs'
    top = restated('checker-24x40', 100)['blocks'][0]
    dc = top[..., 0, 0]
    assert np.abs(top.reshape(-1, 64)[:, 1:]).max() >= 512 and np.abs(np.diff(dc, axis=1)).max() >= 1024
    return sorted(residues), padded_ff
