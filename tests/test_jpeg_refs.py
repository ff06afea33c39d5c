"""``jpeg.jpeg_restatement`` -- the definition of the ``.jpg`` file and the yardstick of ``kgdet_jpeg_encode`` / ``kgdet_jpeg_write``
-- pinned on the CPU: to a float64 reference of its coefficient stage, to a parser of the entropy layer written for the test,
to PIL's decoder, and (a guard against gross errors, not an accuracy claim) to the PSNR of PIL's own encoder.

Figures of a run (``pytest -s`` prints them): of the 508 800 levels of all runs 0.32 % differ from the float64 reference, each
by 1 and each inside the bar; the PSNR of our file and of PIL's against the source, and the two file sizes, are printed per
case by the last test and tabled in the README (demo picture: 47.16 dB / 47.26 dB, 61 592 / 61 359 bytes)."""
import io

import numpy as np
import pytest

from kgdet_amd import jpeg
from tests import jpeg_refs as jr


def test_case_list_covers_what_it_must():
    residues, padded_ff = jr.check_case_list()
    assert residues == list(range(8)) and padded_ff


def test_tables_and_header_layout():
    Q = jpeg.quant_tables(50)
    assert np.array_equal(Q[0], jpeg.BASE_LUMA) and np.array_equal(Q[1], jpeg.BASE_CHROMA)
    assert (jpeg.quant_tables(100) == 1).all() and jpeg.quant_tables(1).max() == 255 and jpeg.quant_tables(1).min() == 255
    assert jpeg.quant_tables(90)[0][0] == 3 and jpeg.quant_tables(25)[0][0] == 32
    for bits, vals in ((jpeg.DC_LUMA_BITS, jpeg.DC_VALS), (jpeg.DC_CHROMA_BITS, jpeg.DC_VALS),
                       (jpeg.AC_LUMA_BITS, jpeg.AC_LUMA_VALS), (jpeg.AC_CHROMA_BITS, jpeg.AC_CHROMA_VALS)):
        assert sum(bits) == len(vals) == len(set(vals))
    assert len(jpeg.AC_LUMA_VALS) == len(jpeg.AC_CHROMA_VALS) == 162
    assert sorted(jpeg.ZIGZAG.tolist()) == list(range(64))
    x = np.arange(8)
    exact = 8192 * np.cos((2 * x[None, :] + 1) * x[:, None] * np.pi / 16) * 0.5
    exact[0] = 8192 * np.sqrt(0.125)
    assert np.array_equal(jpeg.dct_matrix(), np.rint(exact).astype(np.int64))
    assert len(jpeg.header(1, 1, 90)) == jpeg.HEADER_BYTES == 623
    for bad in (0, 101, 50.5):
        with pytest.raises(ValueError):
            jpeg.jpeg_restatement(jr.image('grey-1x1'), bad)
    with pytest.raises(TypeError):
        jpeg.jpeg_restatement(np.zeros((4, 4, 3), dtype=np.float32))
    with pytest.raises(TypeError):
        jpeg.jpeg_restatement(np.zeros((4, 4), dtype=np.uint8))
    assert jpeg.encode_jpeg is not None and 0.7 < jpeg.ERROR_BOUND < 0.74


def test_intermediate_ranges_fit_int32():
    """the extremes of the integer pipeline: saturated pixels in every pattern of the checker case at quality 100"""
    D = np.abs(jpeg.dct_matrix())
    assert (D.sum(axis=1) * 2048).max() < 2 ** 26
    assert (((D.sum(axis=1) * 2048).max() + 1024) >> 11) < 2 ** 15 and D.sum(axis=1).max() * 2 ** 15 < 2 ** 30
    for img in (np.zeros((16, 16, 3), np.uint8), np.full((16, 16, 3), 255, np.uint8), jr.image('checker-16x16')):
        assert max(np.abs(p).max() for p in jpeg.sample_planes(img)) <= 2048
    for name in ('checker-16x16', 'checker-24x40'):
        blocks = jpeg.quantized_blocks(jr.image(name), 100)
        assert max(np.abs(b[..., 0, 0]).max() for b in blocks) <= 1024
        assert max(np.abs(b.reshape(-1, 64)[:, 1:]).max() for b in blocks) <= 1023


_differ = [0, 0]


@pytest.mark.parametrize('name,quality', jr.RUNS)
def test_coefficients_against_float64(name, quality):
    """every level equals the float64 reference's, or differs by exactly 1 where the reference's value before rounding lies
    within E / q of a half-integer (E = ``jpeg.ERROR_BOUND``, counted from the integer pipeline's expressions)"""
    got = jr.restated(name, quality)['blocks']
    ratios = jr.exact_ratios(jr.image(name), quality)
    Q = jpeg.quant_tables(quality)
    for g, r, q in zip(got, ratios, (Q[0], Q[1], Q[1])):
        want = jr.round_half_away(r)
        diff = g != want
        slack = jpeg.ERROR_BOUND / q.reshape(8, 8)
        near_half = np.abs(np.abs(r) - np.floor(np.abs(r)) - 0.5) <= slack
        assert (np.abs(g - want)[diff] == 1).all(), 'a level differs by more than 1'
        assert near_half[diff].all(), 'a level differs away from a rounding boundary'
        _differ[0] += int(diff.sum())
        _differ[1] += diff.size
    print('%s q%d: %d of %d levels differ so far (%.3f %%)' % (name, quality, _differ[0], _differ[1], 100.0 * _differ[0] / _differ[1]))


@pytest.mark.parametrize('name,quality', jr.RUNS)
def test_parser_round_trip_and_header(name, quality):
    parts = jr.restated(name, quality)
    img = jr.image(name)
    got = jr.parse(parts['bytes'])
    assert got['markers'] == [0xD8, 0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA, 0xD9]
    assert got['app0'] == b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00'
    Q = jpeg.quant_tables(quality)
    assert sorted(got['qt']) == [0, 1] and np.array_equal(got['qt'][0], Q[0]) and np.array_equal(got['qt'][1], Q[1])
    assert got['sof'] == (8, img.shape[0], img.shape[1], [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)])
    assert got['sos'] == [(1, 0, 0), (2, 1, 1), (3, 1, 1)] and got['spectral'] == (0, 63, 0)
    assert sorted(got['huff']) == [0x00, 0x01, 0x10, 0x11]
    assert got['bits'] == parts['bits'] and got['stream'] == parts['stream']
    for a, b in zip(got['blocks'], parts['blocks']):
        assert np.array_equal(a, b)
    assert parts['bytes'] == jpeg.jpeg_restatement(img, quality)


def _pil_planes(data, mode):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        assert im.format == 'JPEG' and im.mode == 'RGB'
        size = im.size
        if mode == 'YCbCr':
            im.draft('YCbCr', im.size)
            assert im.mode == 'YCbCr' and im.size == size
        return size, np.array(im)


@pytest.mark.parametrize('name,quality', jr.RUNS)
def test_pil_opens_the_stream(name, quality):
    parts = jr.restated(name, quality)
    img = jr.image(name)
    H, W = img.shape[:2]
    size, ycc = _pil_planes(parts['bytes'], 'YCbCr')
    assert size == (W, H) and ycc.shape == (H, W, 3)
    if name.startswith('checker'):
        return                  # outside IEEE 1180's input range: open / size / mode only
    want = np.clip(np.rint(jr.exact_idct(parts['blocks'][0], jpeg.quant_tables(quality)[0])), 0, 255)[:H, :W]
    worst = np.abs(ycc[..., 0].astype(np.int64) - want.astype(np.int64)).max()
    assert worst <= 1, 'Y plane: %d grey levels from the exact inverse DCT' % worst


def _psnr(a, b):
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


@pytest.mark.parametrize('name', [c[0] for c in jr.CASES])
def test_psnr_is_not_grossly_below_pils(name):
    """a guard, not an accuracy claim: a wrong table, swapped chroma or a shifted block costs many dB"""
    from PIL import Image
    img = jr.image(name)
    ours = jr.restated(name, 90)['bytes']
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format='JPEG', quality=90, subsampling='4:2:0')
    theirs = buf.getvalue()
    a, b = _psnr(_pil_planes(ours, 'RGB')[1], img), _psnr(_pil_planes(theirs, 'RGB')[1], img)
    print('%s: PSNR ours %.2f dB, PIL %.2f dB; %d / %d bytes' % (name, a, b, len(ours), len(theirs)))
    if name.startswith(('noise', 'ramp', 'demo')):
        assert a >= b - 1.0
