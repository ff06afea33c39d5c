"""The ``camera`` switch of the JPEG decoder's definition (kgdet_amd/jpeg.py): 4:2:2 files and restart intervals.

``jpeg.decode_restatement(data, camera=True)`` is held to PIL's decoder (libjpeg-turbo) bit for bit on files PIL wrote; without
the switch ``jpeg.parse_header`` keeps its reasons for the same files; what the switch does not cover keeps a reason with it;
malformed restart files raise ``ValueError``.  The kernels are held to this definition by tests/test_gpu_jpeg_camera.py."""
import numpy as np
import pytest

from kgdet_amd import jpeg
from tests import jpeg_camera_refs as cr
from tests import jpeg_decode_refs as dr


def check_grid(grid):
    seen = set()
    for case in grid:
        data = cr.make(*case)
        assert np.array_equal(jpeg.decode_restatement(data, camera=True), dr.pil(data)), cr.case_name(case)
        frame = cr.frame_of(data)
        seen.add((frame['mode'], frame['restart_interval'] > 0))
    assert seen == {(mode, rst) for mode in (jpeg.MODE_GREY, jpeg.MODE_444, jpeg.MODE_420, jpeg.MODE_422) for rst in (False, True)}


def test_the_definition_equals_pil_on_the_grid():
    assert len(cr.GRID) == 560
    check_grid(cr.GRID)


def test_the_definition_equals_pil_with_optimised_tables_at_the_extreme_qualities():
    assert len(cr.GRID_OPT) == 560 and {c[3] for c in cr.GRID_OPT} == {5, 100}
    check_grid(cr.GRID_OPT)


def test_narrow_422_planes_equal_pil():
    """a chroma row of up to two samples (W <= 4) is replicated by libjpeg, not filtered"""
    for W in (2, 3, 4, 5, 6):
        for restart in (None, ('blocks', 1)):
            data = cr.make('noise', 9, W, 90, '422', restart)
            assert np.array_equal(jpeg.decode_restatement(data, camera=True), dr.pil(data)), (W, restart)


def test_without_the_switch_the_files_keep_their_reasons_and_the_result_its_keys():
    for case in cr.GRID + cr.GRID_OPT:
        data = cr.make(*case)
        frame, reason = cr.frame_of(data), jpeg.parse_header(data)
        if frame['restart_interval']:
            assert isinstance(reason, str) and reason.startswith('restart interval %d (DRI)' % frame['restart_interval']), reason
        elif frame['mode'] == jpeg.MODE_422:
            assert isinstance(reason, str) and reason.startswith('sampling 2x1 / 1x1 / 1x1'), reason
        else:
            assert set(frame) - set(reason) == {'restart_interval'} and frame['restart_interval'] == 0
            assert all(np.array_equal(frame[k], reason[k]) for k in reason)
        if isinstance(reason, str):
            with pytest.raises(ValueError):
                jpeg.decode_restatement(data)
            assert jpeg.parse_header(data, camera=False) == reason
    both = cr.make('noise', 23, 31, 90, '422', ('rows', 1))
    assert jpeg.parse_header(both).startswith('restart interval')


def sof_patched(data, sampling):
    """``data`` with the luma sampling byte of its SOF0 replaced"""
    at = data.index(b'\xff\xc0')
    assert data[at + 9] == 3 and data[at + 11] in (0x11, 0x21, 0x22)
    return data[:at + 11] + bytes([sampling]) + data[at + 12:]


def test_with_the_switch_everything_else_keeps_a_reason():
    data = cr.make('noise', 23, 31, 90, '422')
    assert jpeg.parse_header(sof_patched(data, 0x12), camera=True).startswith('sampling 1x2 / 1x1 / 1x1')
    assert jpeg.parse_header(sof_patched(data, 0x41), camera=True).startswith('sampling 4x1 / 1x1 / 1x1')
    assert jpeg.parse_header(sof_patched(data, 0x21), camera=True)['mode'] == jpeg.MODE_422
    progressive = dr.write_jpeg(dr.GENERATORS['noise'](16, 16, 0), 90, '420', progressive=True, restart_marker_rows=1)
    assert 'progressive' in jpeg.parse_header(progressive, camera=True)
    for patched in (sof_patched(data, 0x12), sof_patched(data, 0x41), progressive):
        with pytest.raises(ValueError):
            jpeg.decode_restatement(patched, camera=True)
    adobe = dr.insert_segments(data, [b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01'])
    assert 'Adobe' in jpeg.parse_header(adobe, camera=True)


@pytest.mark.parametrize('kind', ['420', '422', '444', 'grey'])
def test_malformed_restart_files_raise(kind):
    good = cr.make('noise', 40, 56, 90, kind, ('blocks', 2))
    assert np.array_equal(jpeg.decode_restatement(good, camera=True), dr.pil(good))
    bad = cr.broken(good)
    assert set(bad) == {'swapped', 'missing', 'surplus', 'out_of_order', 'cut_short'}
    for name, data in bad.items():
        with pytest.raises(ValueError):
            jpeg.decode_restatement(data, camera=True)
    # a second 0xFF in front of a marker is no fill byte: it ends the scan
    at = cr.markers(good)[1][0]
    with pytest.raises(ValueError, match='FF ends the scan'):
        jpeg.decode_restatement(good[:at] + b'\xff' + good[at:], camera=True)


def test_the_marker_number_wraps_after_eight_intervals():
    data = cr.make('noise', 33, 130, 90, '422', ('blocks', 1))
    found = [m for _, m in cr.markers(data)]
    assert len(found) == 9 * 5 - 1 and found == [k % 8 for k in range(len(found))]
    parts = jpeg.decode_parts(data, camera=True)
    assert len(parts['intervals']) == 45 and sum(parts['intervals']) == len(parts['stream'])
    assert np.array_equal(parts['image'], dr.pil(data))


def test_an_interval_of_at_least_all_mcus_has_no_marker():
    for blocks in (12, 13, 500):                                # 40 x 56 at 4:2:0: 3 x 4 MCUs
        data = cr.make('ramp', 40, 56, 90, '420', ('blocks', blocks))
        assert cr.frame_of(data)['restart_interval'] == blocks and cr.markers(data) == []
        assert np.array_equal(jpeg.decode_restatement(data, camera=True), dr.pil(data))
    with pytest.raises(ValueError):                             # and a marker in such a file is one too many
        one = cr.make('ramp', 40, 56, 90, '420', ('blocks', 6))
        at = one.index(b'\xff\xdd')
        jpeg.decode_restatement(one[:at + 4] + b'\x00\x0c' + one[at + 6:], camera=True)
