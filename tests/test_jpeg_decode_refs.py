"""``jpeg.decode_restatement`` against PIL's decoder, ``jpeg.parse_header`` on the files it takes and refuses, and what the GPU
tests' case list puts on the Huffman kernel's subsequence boundaries (CPU only)."""
import numpy as np
import pytest

from kgdet_amd import jpeg
from tests import jpeg_decode_refs as dr
from tests import jpeg_refs


# ---- the restatement against PIL ---------------------------------------------------------------------------------------------
def test_the_72_files_of_the_definition_equal_pil():
    assert len(dr.CASES_72) == 72
    for case in dr.CASES_72:
        data = dr.make(*case)
        assert np.array_equal(jpeg.decode_restatement(data), dr.pil(data)), dr.case_name(case)


def test_444_one_component_and_optimised_tables_equal_pil():
    assert {c[4] for c in dr.CASES_KINDS} == {'444', 'grey', '420-opt', '444-opt', 'grey-opt'}
    modes, standard = set(), set()
    for case in dr.CASES_KINDS:
        data = dr.make(*case)
        parts = jpeg.decode_parts(data)
        modes.add(parts['frame']['mode'])
        standard.add(parts['frame']['ac'][0][0] == jpeg.AC_LUMA_BITS)
        assert np.array_equal(parts['image'], dr.pil(data)), dr.case_name(case)
    assert modes == {jpeg.MODE_GREY, jpeg.MODE_444, jpeg.MODE_420} and standard == {True, False}


def test_the_gpu_cases_equal_pil():
    for case in dr.GPU_CASES + dr.UNIFORM_CASES[:1]:
        assert np.array_equal(dr.restated(case)['image'], dr.pil(dr.make(*case))), dr.case_name(case)


def test_the_demo_image_equals_pil():
    data = dr.demo_file()
    parts = jpeg.decode_parts(data)
    assert parts['image'].shape == (624, 468, 3) and parts['frame']['mode'] == jpeg.MODE_420
    assert np.array_equal(parts['image'], dr.pil(data))
    assert np.array_equal(parts['image'], jpeg_refs.demo(624, 468, 0))


def test_the_restatement_reads_the_encoder_restatement():
    """the file ``jpeg.jpeg_restatement`` defines, decoded: the levels are the encoder's, the picture is PIL's"""
    img = jpeg_refs.image('noise-80x96')
    parts = jpeg_refs.restated('noise-80x96', 90)
    got = jpeg.decode_parts(parts['bytes'])
    Y, Cb, Cr = parts['blocks']
    mh, mw = Cb.shape[:2]
    coef = got['coefficients'].reshape(mh, mw, 6, 8, 8)
    assert np.array_equal(coef[:, :, 4], Cb) and np.array_equal(coef[:, :, 5], Cr)
    assert np.array_equal(coef[:, :, :4].reshape(mh, mw, 2, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(2 * mh, 2 * mw, 8, 8), Y)
    assert np.array_equal(got['image'], dr.pil(parts['bytes'])) and got['image'].shape == img.shape


def test_a_patched_dc_table_entry_is_outside_the_pinned_domain_but_defined():
    """quantiser entry 40 on the DC: both clamp.  Entry 255: PIL's inverse DCT wraps (not asserted: unpinned), the definition clamps"""
    img = np.full((16, 16, 3), 255, np.uint8)
    img[:8] = 0
    data = bytearray(dr.write_jpeg(img, 100, '420'))
    k = data.find(b'\xff\xdb')
    for entry in (40, 255):
        data[k + 5] = entry
        got = jpeg.decode_restatement(bytes(data))
        assert (got[0, 0] == 0).all() and (got[15, 15] == 255).all()
        if entry == 40:
            assert np.array_equal(got, dr.pil(bytes(data)))


def test_malformed_scans_raise():
    good = dr.make('noise', 33, 47, 90, '420')
    start = dr.scan_start(good)
    for bad in (good[:-2], good[:start + 40], good[:start + 40] + b'\xff\xd9', good[:start + 40] + b'\xff\xd0' + good[start + 40:]):
        with pytest.raises(ValueError):
            jpeg.decode_restatement(bad)
    assert np.array_equal(jpeg.decode_restatement(good + b'trailing bytes'), dr.pil(good))       # bytes after EOI are ignored


# ---- parse_header --------------------------------------------------------------------------------------------------------------
def test_parse_header_describes_the_frame():
    for case, mode in ((('noise', 33, 47, 90, '420'), jpeg.MODE_420), (('noise', 33, 47, 90, '444'), jpeg.MODE_444),
                       (('noise', 33, 47, 90, 'grey'), jpeg.MODE_GREY)):
        data = dr.make(*case)
        frame = jpeg.parse_header(data)
        assert (frame['H'], frame['W'], frame['mode']) == (33, 47, mode)
        assert data[frame['scan_offset'] - 3:frame['scan_offset']] == b'\x00\x3f\x00'
        assert len(frame['tables']) == jpeg.DECODE_TABLE_BYTES == 1024
        ref = jpeg_refs.parse(data)['qt'] if mode == jpeg.MODE_420 else None
        if ref is not None:
            assert np.array_equal(frame['qt'][0], ref[0]) and np.array_equal(frame['qt'][1], ref[1]) and np.array_equal(frame['qt'][2], ref[1])
        assert bytes(frame['tables'][:64]) == frame['qt'][0].tobytes() and list(frame['tables'][192:208]) == frame['dc'][0][0]
        blocks = {jpeg.MODE_420: (3, 3, 6), jpeg.MODE_444: (6, 5, 3), jpeg.MODE_GREY: (6, 5, 1)}[mode]
        assert jpeg.frame_blocks(frame) == blocks           # a one-component scan: ceil(W / 8) blocks per row


def test_parse_header_takes_merged_tables_comments_app_segments_and_fill_bytes():
    data = dr.make('ramp', 33, 47, 50, '420-opt')
    ref = dr.pil(data)
    merged = dr.merge_tables(dr.merge_tables(data, 0xDB), 0xC4)
    assert merged.count(b'\xff\xdb') == 1 and merged.count(b'\xff\xc4') == 1 and merged != data
    com = b'\xff\xfe\x00\x0ba comment'
    app = b'\xff\xe1\x00\x08Exif\x00\x00' + b'\xff\xed\x00\x04\xff\xd9'         # (marker bytes inside a segment are not markers)
    fill = b'\xff\xff\xff'
    variants = dict(merged=merged, comment=dr.insert_segments(data, [com]), app=dr.insert_segments(data, [app, com], 0xC0),
                    fill=dr.insert_segments(merged, [fill], 0xC0), fill_and_comment=dr.insert_segments(data, [fill, com, fill], 0xC4),
                    dri_zero=dr.insert_segments(data, [b'\xff\xdd\x00\x04\x00\x00'], 0xDA))
    for name, variant in variants.items():
        frame = jpeg.parse_header(variant)
        assert not isinstance(frame, str), (name, frame)
        assert np.array_equal(jpeg.decode_restatement(variant), ref), name
        if 'fill' not in name:                              # (PIL reads these; fill bytes in front of a marker it reads too)
            assert np.array_equal(dr.pil(variant), ref), name


def test_parse_header_gives_a_reason_for_every_refused_kind():
    img = dr.GENERATORS['noise'](32, 32, 0)
    base = dr.write_jpeg(img, 90, '420')
    from PIL import Image
    import io
    cmyk = io.BytesIO()
    Image.fromarray(img).convert('CMYK').save(cmyk, 'JPEG', quality=90)
    sof = base.find(b'\xff\xc0')
    dqt = base.find(b'\xff\xdb')

    def patched(at, value):
        out = bytearray(base)
        out[at] = value
        return bytes(out)
    wide_table = base[:dqt] + b'\xff\xdb\x00\x83\x10' + bytes(128) + base[dqt:]
    refused = dict(
        progressive=(dr.write_jpeg(img, 90, '420', progressive=True), 'progressive'),
        sampling_422=(dr.write_jpeg(img, 90, '420', subsampling=1), 'sampling'),
        restart=(dr.write_jpeg(img, 90, '420', restart_marker_blocks=2), 'restart interval'),
        cmyk=(cmyk.getvalue(), 'Adobe'),
        extended=(patched(sof + 1, 0xC1), 'extended'), lossless=(patched(sof + 1, 0xC3), 'lossless'),
        arithmetic=(patched(sof + 1, 0xC9), 'arithmetic'), twelve_bit=(patched(sof + 4, 12), '12-bit'),
        sixteen_bit_table=(wide_table, '16-bit quantisation'),
        four_components=(base[:sof] + b'\xff\xc0\x00\x14\x08\x00\x20\x00\x20\x04\x01\x11\x00\x02\x11\x00\x03\x11\x00\x04\x11\x00'
                         + base[sof + 19:], 'four components'),
        dnl=(patched(sof + 5, 0)[:sof + 6] + b'\x00' + base[sof + 7:], 'H = 0'),
        adobe=(dr.insert_segments(base, [b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01'], 0xDB), 'APP14'),
        second_scan=(base[:base.find(b'\xff\xda')] + b'\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00' + base[dr.scan_start(base):],
                     'more than one scan'),
        scan_of_other_ids=(patched(sof + 10, ord('R')), 'scan names component'),
        not_jpeg=(b'\x89PNG\r\n\x1a\n' + bytes(32), 'SOI'), truncated=(base[:sof + 6], 'runs past'),
        no_tables=(base[:dqt] + base[sof:], 'does not define'))
    for name, (data, word) in refused.items():
        reason = jpeg.parse_header(data)
        assert isinstance(reason, str) and word in reason, (name, reason)
        with pytest.raises(ValueError):
            jpeg.decode_restatement(data)
    assert not isinstance(jpeg.parse_header(base), str)
    # three components without JFIF count as YCbCr by their ids 1, 2, 3 -- and not with other ids
    no_jfif = base[:2] + base[20:]
    assert base[2:4] == b'\xff\xe0' and base[4:6] == b'\x00\x10' and not isinstance(jpeg.parse_header(no_jfif), str)
    k = no_jfif.find(b'\xff\xc0')
    other_ids = bytearray(no_jfif)
    other_ids[k + 10] = ord('R')
    s = no_jfif.find(b'\xff\xda')
    other_ids[s + 5] = ord('R')
    assert 'not marked as YCbCr' in jpeg.parse_header(bytes(other_ids))


# ---- the subsequence boundaries ------------------------------------------------------------------------------------------------
def test_the_gpu_cases_put_every_kind_of_cut_on_a_boundary():
    S = jpeg.DECODE_SUBSEQ_BITS
    total = dict.fromkeys(dr.CENSUS_KEYS, 0)
    for case in dr.GPU_CASES:
        census = dr.boundary_census(dr.make(*case), S)
        for key in dr.CENSUS_KEYS:
            total[key] += census[key]
    assert all(total[key] > 0 for key in dr.CENSUS_KEYS), total


def test_the_census_counts_what_it_says():
    """a hand-made trace: one boundary inside a code, one inside magnitude bits, a block that ends on a boundary"""
    data = dr.make('noise', 8, 8, 100, 'grey')
    trace = []
    parts = jpeg.decode_parts(data, trace)
    assert sum(1 for t in trace if t[5]) == 1 and trace[0][3] == -1 and trace[0][0] == 0
    bits = trace[-1][0] + trace[-1][1] + trace[-1][2]
    assert 0 <= parts['context'].total_bits - bits < 8
    for S in (8, 16, 64):
        census = dr.boundary_census(data, S)
        codes = sum(1 for p, n, s, _, _, _ in trace if (p + n - 1) // S > p // S)
        assert census['code_straddles'] == codes and census['block_over_two_boundaries'] == (1 if (bits - 1) // S >= 2 else 0)
        assert census['block_ends_on_boundary'] == (1 if bits % S == 0 else 0)


def test_uniform_pictures_hold_a_long_run_a_cold_start_does_not_synchronise_in():
    for case in dr.UNIFORM_CASES:
        assert dr.cold_run(dr.make(*case)) >= 16, dr.case_name(case)


def test_the_fixpoint_of_cold_starts_is_the_true_parse():
    """the kernel's scheme in plain Python, with short chunks so that several follow each other"""
    for case in (dr.GPU_CASES[100], dr.GPU_CASES[130], dr.GPU_CASES[143], dr.UNIFORM_CASES[0], ('ramp', 80, 96, 90, '420')):
        data = dr.make(*case)
        parts = jpeg.decode_parts(data)
        frame = parts['frame']
        coef, rounds, final, blocks = dr.fixpoint_decode(data, jpeg.DECODE_SUBSEQ_BITS, 8)
        assert blocks == len(parts['coefficients']) and final[2] == 0 and 0 <= parts['context'].total_bits - final[0] < 8
        assert np.array_equal(coef[:, 1:], parts['coefficients'][:, 1:]), dr.case_name(case)
        mw, mh, bpm = jpeg.frame_blocks(frame)
        dc = coef[:, 0].reshape(mw * mh, bpm)
        for slots in {jpeg.MODE_GREY: ((0,),), jpeg.MODE_444: ((0,), (1,), (2,)), jpeg.MODE_420: ((0, 1, 2, 3), (4,), (5,))}[frame['mode']]:
            part = dc[:, slots]
            assert np.array_equal(np.cumsum(part.reshape(-1)).reshape(part.shape), parts['coefficients'][:, 0].reshape(mw * mh, bpm)[:, slots])
        assert all(1 <= r <= 9 for r in rounds)
    assert max(dr.fixpoint_decode(dr.make(*dr.UNIFORM_CASES[0]))[1]) >= 17
