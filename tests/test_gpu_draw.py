"""``kgdet_draw_detections`` (csrc/draw.hip) through the C ABI.

The bar is EQUALITY of bytes with ``visualize.draw_restatement`` (held to independent formulations on the CPU by
tests/test_draw_refs.py).  The destination is pre-filled with 0xAA between 64-byte canaries: every byte of an image must be
written, nothing beside it, and the source must come back unchanged."""
import ctypes

import numpy as np
import pytest
import torch

from kgdet_amd import _lib
from kgdet_amd import visualize as vz
from kgdet_amd.evaluation import landmark_meta
from tests import draw_cases as dc

pytestmark = pytest.mark.gpu
i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
FILL, CANARY, PAD = 0xAA, 0x5C, 64


def launch(images, block, style, shift=0, blocks=None, override=()):
    """``images`` drawn from ``block`` [n, M, 7 + 3K] in ONE launch; image i's destination starts at an address that is
    ``shift`` (+ 4 i) mod 16 -> (status, the drawn arrays).  Asserts the canaries, the fill between the images and the source."""
    n = len(images)
    st = vz.Style(style.pop('class_names'), **style)
    src_at, dst_at, s_total, d_total = [], [], 0, PAD
    for i, img in enumerate(images):
        src_at.append(s_total + (3 * i) % 5)                             # (unaligned sources too)
        s_total = src_at[-1] + img.size + 7
        want = (shift + 4 * i) % 16
        d_total += (want - d_total) % 16
        dst_at.append(d_total)
        d_total += img.size + 5
    d_total += PAD
    src_host = np.full(s_total, 0x33, dtype=np.uint8)
    for img, at in zip(images, src_at):
        src_host[at:at + img.size] = img.reshape(-1)
    src = torch.from_numpy(src_host).cuda()
    dst = torch.full((d_total,), FILL, dtype=torch.uint8, device='cuda')
    dst[:PAD] = CANARY
    dst[-PAD:] = CANARY
    assert dst.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
    rows = torch.from_numpy(np.ascontiguousarray(block, dtype=np.float32)).cuda()

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    offsets = np.concatenate([[0], np.cumsum([len(b) for b in st.names])]).astype(np.int32)
    names = up(np.frombuffer(b''.join(st.names) + b'\0', dtype=np.uint8).copy())
    colors, name_off, glyphs = up(st.colors), up(offsets), up(st.glyphs)
    ranges = None if st.ranges is None else up(st.ranges)
    table = (i64 * (4 * n))(*[v for i in range(n) for v in (src_at[i], dst_at[i], images[i].shape[0], images[i].shape[1])])
    blk = (i32 * n)(*(list(range(n)) if blocks is None else blocks))
    p = _lib.ptr
    a = dict(src=p(src), src_bytes=s_total, dst=p(dst), dst_bytes=d_total, table=table, blk=blk, n=n, rows=p(rows),
             N=rows.shape[0], M=rows.shape[1], W7=rows.shape[2], colors=p(colors), L=st.L, names=p(names), name_off=p(name_off),
             name_total=int(offsets[-1]), ranges=p(ranges), glyphs=p(glyphs), thr=float(st.score_thr), t=st.thickness,
             radius=st.radius, contour=int(st.contour), lw=st.line_width, s=st.font_scale,
             kpt=-1 if st.kpt_color is None else (st.kpt_color[0] << 16 | st.kpt_color[1] << 8 | st.kpt_color[2]))
    a.update(override)
    rc = _lib.lib().kgdet_draw_detections(
        a['src'], i64(a['src_bytes']), a['dst'], i64(a['dst_bytes']), a['table'], a['blk'], i32(a['n']), a['rows'], i64(a['N']),
        i32(a['M']), i32(a['W7']), a['colors'], i32(a['L']), a['names'], a['name_off'], i32(a['name_total']), a['ranges'],
        a['glyphs'], ctypes.c_float(a['thr']), i32(a['t']), i32(a['radius']), i32(a['contour']), i32(a['lw']), i32(a['s']),
        i32(a['kpt']), _lib.current_stream())
    host = dst.cpu().numpy()
    assert (host[:PAD] == CANARY).all() and (host[-PAD:] == CANARY).all(), 'a canary was overwritten'
    assert np.array_equal(src.cpu().numpy(), src_host), 'the source was written'
    mask = np.ones(d_total, dtype=bool)
    mask[:PAD] = mask[-PAD:] = False
    out = []
    for img, at in zip(images, dst_at):
        mask[at:at + img.size] = False
        out.append(host[at:at + img.size].reshape(img.shape))
    assert (host[mask] == FILL).all(), 'bytes beside the images were written'
    return rc, out


def check(images, block, shift=0, blocks=None, **style):
    """the launch against the restatement, image by image; returns the drawn arrays"""
    names = style.pop('class_names', dc.NAMES3)
    rc, got = launch(images, block, dict(style, class_names=names), shift, blocks)
    assert rc == 0, _lib.lib().kgdet_last_error()
    for i, img in enumerate(images):
        rows = block[i if blocks is None else blocks[i]]
        want = vz.draw_restatement(img, rows, vz.row_count(rows), names, **style)
        bad = np.argwhere((got[i] != want).any(axis=2))
        assert len(bad) == 0, 'image %d: %d pixels differ, first at (y, x) = %s' % (i, len(bad), bad[0])
    return got


SIZES = [(1, 1), (7, 5), (33, 65), (70, 100)]           # (H, W): partial tiles, 3 W no multiple of 4


@pytest.mark.parametrize('shift', [0, 1, 2, 3, 4, 8, 12])
def test_image_sizes_and_destination_alignment(shift):
    """four images in one launch; with ``shift`` 0 .. 3 their destinations lie at shift, shift + 4, + 8, + 12 mod 16"""
    images = [dc.image(H, W, seed=k) for k, (H, W) in enumerate(SIZES)]
    block = np.stack([dc.random_rows(shift * 10 + k, 12, 3, H, W, 3) for k, (H, W) in enumerate(SIZES)])
    got = check(images, block, shift, contour=True)
    assert any((g != img).any() for g, img in zip(got, images))


def test_three_sizes_in_one_launch_one_without_detections():
    sizes = [(40, 130), (70, 100), (17, 64)]
    images = [dc.image(H, W, seed=10 + k) for k, (H, W) in enumerate(sizes)]
    block = np.stack([dc.random_rows(50 + k, 9, 3, H, W, 3, count=(0 if k == 1 else 9)) for k, (H, W) in enumerate(sizes)])
    got = check(images, block, 5, contour=True)
    assert np.array_equal(got[1], images[1]) and (got[0] != images[0]).any() and (got[2] != images[2]).any()
    swapped = check(images, block, 0, blocks=[2, 2, 0])          # (the image's row block is the table's, not its place)
    assert (swapped[1] != images[1]).any()


@pytest.mark.parametrize('M', [1, 7, 100, 1024])
def test_row_block_sizes_and_counts(M):
    H, W = 70, 100
    img = dc.image(H, W, seed=M)
    for count in sorted(set([0, 1, M])):
        got = check([img], dc.awkward_rows(M, H, W, 3, count)[None], 0, contour=True)[0]
        assert (count == 0) == np.array_equal(got, img)
    over = dc.awkward_rows(M, H, W, 3, M)
    over[:, 6] = M + 5                                            # (a count beyond the block is cut to M)
    check([img], over[None])


def test_rows_that_draw_nothing_leave_the_source():
    H, W = 33, 65
    img = dc.image(H, W, seed=3)
    rows = dc.random_rows(4, 8, 3, H, W, 3)
    rows[:, 4] = 0.9
    rows[0, 0], rows[1, 5], rows[2, 5], rows[3, 5], rows[4, 4], rows[5, 4] = np.nan, -1, 3, 2.5, np.float32(0.3), 0.2
    rows[6, 3], rows[7, 4] = -np.inf, np.nan
    assert np.array_equal(check([img], rows[None])[0], img)


@pytest.mark.parametrize('thickness', [1, 2, 5])
def test_box_geometry(thickness):
    H, W = 70, 100
    img = dc.image(H, W, seed=20)
    got = check([img], dc.box_rows(H, W)[None], 3, thickness=thickness)[0]
    assert (got != img).any()


@pytest.mark.parametrize('radius,line_width,font_scale', [(1, 1, 1), (2, 2, 3), (64, 16, 1), (3, 5, 8)])
def test_discs_capsules_and_labels(radius, line_width, font_scale):
    H, W = 70, 100
    img = dc.image(H, W, seed=30)
    for kpt_color in (vz.KPT_COLOR, None):
        check([img], dc.landmark_rows(H, W)[None], 2, radius=radius, line_width=line_width, font_scale=font_scale, contour=True,
              kpt_color=kpt_color)
    check([img], dc.landmark_rows(H, W)[None], 2, radius=radius, font_scale=font_scale)             # (no contour)


def test_deepfashion2_ranges_draw_only_the_category():
    meta = landmark_meta()
    names, ranges = meta['classes'], meta['landmark_ranges']
    H, W = 70, 100
    img = dc.image(H, W, seed=40)
    rows = dc.random_rows(41, 13, 294, H, W, len(names))
    rows[:, 4], rows[:, 5] = 0.9, np.arange(13)
    got = check([img], rows[None], 1, class_names=names, landmark_ranges=ranges, contour=True)[0]
    everything = vz.draw_restatement(img, rows, 13, names, contour=True)
    assert (got != everything).any()                              # (without ranges all 294 would appear)
    check([img], rows[None], 1, class_names=names, contour=True, radius=1)     # K = 294 without ranges: five chunks of 64


def test_labels_clipped_moved_inside_and_unknown_bytes():
    H, W = 70, 100
    img = dc.image(H, W, seed=50)
    rows = dc.empty_rows(6, 3)
    dc.set_row(rows, 0, (60, 30, 95, 60), 0.999, 1)               # the text runs past the right edge
    dc.set_row(rows, 1, (10, 4, 50, 20), 0.125, 0)                # no room above: inside the box
    dc.set_row(rows, 2, (-30, 50, 20, 66), 9.996, 2)              # starts left of the image; the digits saturate at 9.99
    dc.set_row(rows, 3, (40, 9, 70, 25), 0.375, 0)                # top edge exactly on row 0
    dc.set_row(rows, 4, (5, 69, 30, 80), 0.625, 1)                # only the label reaches the image
    dc.finish(rows, 5)
    for s in (1, 3):
        check([img], rows[None], 0, font_scale=s, score_thr=0.1)
    check([img], rows[None], 0, class_names=['café!', '', 'x' * 255], score_thr=0.1)          # blocks, no name, 255 bytes


def test_order_later_rows_and_upper_layers_win():
    H, W = 48, 96
    img = dc.image(H, W, seed=60)
    rows = dc.empty_rows(3, 3)
    dc.set_row(rows, 0, (20, 20, 80, 40), 0.9, 0, [(22, 12, 1), (40, 12, 1), (0, 0, 0)])
    dc.set_row(rows, 1, (18, -20, 60, 30), 0.8, 1)                # its right edge (x = 59, 60) crosses row 0's label (rows 11 .. 19)
    dc.finish(rows, 2)
    got = check([img], rows[None], 0, contour=True)[0]
    colors = vz.palette(3)
    assert tuple(got[12, 59]) == tuple(got[12, 60]) == tuple(colors[1])
    assert tuple(got[11, 58]) == tuple(got[11, 61]) == tuple(colors[0])       # (the label's empty top line beside it)
    one = dc.empty_rows(1, 3)
    dc.set_row(one, 0, (10, 8, 60, 40), 0.9, 2, [(10, 8, 1), (14, 8, 1), (0, 0, 0)])      # box, contour, disc and label at (10, 8)
    dc.finish(one, 1)
    got = check([img], one[None], 0, contour=True, thickness=3)[0]
    assert tuple(got[8, 10]) == tuple(got[8, 14]) == tuple(colors[2])          # the label, moved inside, is on top

def test_refusals_return_shape_errors_and_write_nothing():
    H, W = 33, 65
    img = dc.image(H, W, seed=70)
    block = dc.random_rows(71, 7, 3, H, W, 3)[None]
    null = vp(0)

    def tab(h, w):
        return (i64 * 4)(0, PAD, h, w)
    cases = [dict(M=0), dict(M=1025), dict(W7=11), dict(W7=7), dict(W7=7 + 3 * 1025), dict(L=0), dict(L=65), dict(n=-1), dict(n=33),
             dict(t=0), dict(t=65), dict(radius=0), dict(radius=65), dict(lw=0), dict(lw=17), dict(s=0), dict(s=9), dict(kpt=-2),
             dict(kpt=1 << 24), dict(table=tab(0, W)), dict(table=tab(H, 0)), dict(table=tab(8193, 1)), dict(table=tab(1, 8193)),
             dict(table=(i64 * 4)(-1, PAD, H, W)), dict(table=(i64 * 4)(0, -1, H, W)), dict(table=(i64 * 4)(8, PAD, H, W)),
             dict(table=(i64 * 4)(0, PAD + 70, H, W)), dict(blk=(i32 * 1)(1)), dict(blk=(i32 * 1)(-1)), dict(N=-1),
             dict(src=null), dict(dst=null), dict(table=null), dict(blk=null), dict(rows=null), dict(colors=null), dict(names=null),
             dict(name_off=null), dict(glyphs=null), dict(src_bytes=-1), dict(dst_bytes=-1)]
    for kw in cases:
        rc, out = launch([img], block, dict(class_names=dc.NAMES3), 0, override=kw)
        assert rc == _lib.KGDET_E_SHAPE, kw
        assert (out[0] == FILL).all(), kw
    rc, out = launch([img], block, dict(class_names=dc.NAMES3), 0, override=dict(n=0, table=null))
    assert rc == 0 and (out[0] == FILL).all()
    src = torch.zeros(3 * H * W + 64, dtype=torch.uint8, device='cuda')               # in place: refused
    rc, out = launch([img], block, dict(class_names=dc.NAMES3), 0,
                     override=dict(src=_lib.ptr(src), dst=_lib.ptr(src), src_bytes=src.numel(), dst_bytes=src.numel(),
                                   table=(i64 * 4)(0, 0, H, W)))
    assert rc == _lib.KGDET_E_SHAPE and (src.cpu().numpy() == 0).all()
