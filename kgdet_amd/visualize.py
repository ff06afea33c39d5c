"""Detections and landmarks drawn on images: ``show_result``, ``DeviceDrawer`` and the definition of the picture.

The reference draws with ``mmcv.imshow_det_bboxes`` (``mmdet/apis/inference.py:104-160``, ``mmdet/models/detectors/base.py:90-142``)
and with cv2 (``tools/visualization.py``); neither library exists here and neither draws a KGDet result's landmarks, so the
picture is defined in this file, once, by ``draw_restatement`` (numpy).  It is the CPU fallback of the public functions and
the yardstick of ``kgdet_draw_detections`` (csrc/draw.hip), which is held to it bit for bit.  cv2's and mmcv's own pixels are
unpinned.

The picture
-----------
``image`` uint8 [H, W, 3] RGB, 1 <= H, W <= 8192; ``rows`` float32 [M, 7 + 3K] in the layout of ``decode.pack_rows`` (box 4,
score, label, count, K x (x, y, v)); only rows r < ``count`` are read.  Row r is drawn when ``score > score_thr`` (compared in
float32, strictly, as mmcv does), its label is an integer in [0, L) and its four box values are finite.  A coordinate is
``np.rint`` of the float32 value (half to even), clamped to [-8192, 16383].  A pixel is the point (x, y) of its indices.

Layers of a row, bottom to top:

0. box: x0 <= x <= x1, y0 <= y <= y1 and (x < x0 + t or x > x1 - t or y < y0 + t or y > y1 - t), t = ``thickness``, in the
   class colour; an empty box (x1 < x0 or y1 < y0) draws nothing.  For a box at least 2t on a side this is PIL's
   ``ImageDraw.rectangle(outline, width=t)``.
1. contour (``contour=True``): for consecutive landmarks k, k + 1 of the category's range, both with v > 0 and finite
   coordinates, the capsule of half-width ``line_width / 2`` around P -> Q, in doubled coordinates (X2 = 2X) so that all is
   integer: d = Q2 - P2, v = X2 - P2, R2 = line_width ** 2; v.d <= 0: |v|^2 <= R2; v.d >= d.d: |X2 - Q2|^2 <= R2; else
   cross(v, d)^2 <= R2 * d.d.  Class colour.
2. landmarks: for every landmark of the range [a, b) with v > 0 and finite coordinates the disc (x - cx)^2 + (y - cy)^2 <=
   radius^2, in ``kpt_color`` (None: the class colour).  The range is ``landmark_ranges[label]`` cut to [0, K]; without ranges
   all K landmarks.
3. label: ``name|d.dd`` (mmcv's ``'{}|{:.02f}'``), digits from q = clamp(rint(float64(score) * 100), 0, 999) -- the product is
   exact in float64, so this is ``'%.2f'`` for every float32 score in [0, 9.995).  Glyphs are the 5 x 7 bitmaps of ``GLYPHS``
   (a byte without one is a solid block) in cells of 6s x 9s pixels, s = ``font_scale``: one empty column before each glyph
   and one after the last, one empty line above and below.  The text box, (6n + 1)s wide and 9s tall, is filled with the class
   colour; glyph pixels are black where 299 R + 587 G + 114 B >= 128000 for that colour, else white.  Its left edge is x0, its
   bottom edge row y0 - 1; where that would start above row 0 its top edge is y0.  A class name is at most 255 bytes (UTF-8).

A pixel shows the covering primitive with the greatest (r, layer): rows in index order, later over earlier, as mmcv's loop
draws them.  A pixel nothing covers keeps its source value.  Nothing is blended, so the order of evaluation does not matter.

Integer ranges: coordinates lie in [-8192, 16383], pixels in [0, 8191], so in doubled units every component of d is at most
2 * 24575 and of v at most 2 * 16383 + 1 in magnitude.  cross(v, d) is four times twice the area of the triangle P, Q, X,
whose corners lie in a square of side 24575: |cross| <= 4 * 24575^2 < 2^31.2 and its square is below 2^62.4; d.d <= 8 *
24575^2 < 2^32.2 and R2 <= 256, so R2 * d.d < 2^40.2; v.d and |v|^2 stay below 2^33.  Everything fits int64.
"""
import os
from collections import deque

import numpy as np

COORD_MIN, COORD_MAX, MAX_SIDE = -8192, 16383, 8192
MAX_NAME_BYTES = 255
MAX_IMAGES = 32             # KGDET_DRAW_MAX_IMAGES: images of one launch
KPT_COLOR = (255, 0, 0)     # the reference's red dots (tools/visualization.py)

# 5 x 7 glyphs: seven row masks per character, top to bottom, bit 4 = the left column
GLYPHS = {
    ' ': '00000000000000', '.': '00000000000C0C', '_': '0000000000001F', '|': '04040404040404', '-': '0000001F000000',
    '0': '0E11131519110E', '1': '040C040404040E', '2': '0E11010204081F', '3': '1F02040201110E', '4': '02060A121F0202',
    '5': '1F101E0101110E', '6': '0608101E11110E', '7': '1F010204080808', '8': '0E11110E11110E', '9': '0E11110F01020C',
    'A': '0E11111F111111', 'B': '1E11111E11111E', 'C': '0E11101010110E', 'D': '1C12111111121C', 'E': '1F10101E10101F',
    'F': '1F10101E101010', 'G': '0E11101711110F', 'H': '1111111F111111', 'I': '0E04040404040E', 'J': '0702020202120C',
    'K': '11121418141211', 'L': '1010101010101F', 'M': '111B1515111111', 'N': '11111915131111', 'O': '0E11111111110E',
    'P': '1E11111E101010', 'Q': '0E11111115120D', 'R': '1E11111E141211', 'S': '0F10100E01011E', 'T': '1F040404040404',
    'U': '1111111111110E', 'V': '11111111110A04', 'W': '1111111515150A', 'X': '11110A040A1111', 'Y': '11110A04040404',
    'Z': '1F01020408101F',
    'a': '00000E010F110F', 'b': '10101619111116', 'c': '00000E1010110E', 'd': '01010D1311110F', 'e': '00000E111F100E',
    'f': '0609081C080808', 'g': '000F11110F010E', 'h': '10101619111111', 'i': '04000C0404040E', 'j': '0200060202120C',
    'k': '10101214181412', 'l': '0C04040404040E', 'm': '00001A15151111', 'n': '00001619111111', 'o': '00000E1111110E',
    'p': '001E11111E1010', 'q': '000D13110F0101', 'r': '00001619101010', 's': '00000E100E011E', 't': '08081C08080906',
    'u': '0000111111130D', 'v': '00001111110A04', 'w': '0000111115150A', 'x': '0000110A040A11',
    'y': '001111110F010E', 'z': '00001F0204081F',
}
BLOCK = 0x1F                # every row of a byte without a glyph


def glyph_table():
    """uint8 [256, 7]: the row masks of every byte"""
    table = np.full((256, 7), BLOCK, dtype=np.uint8)
    for ch, rows in GLYPHS.items():
        table[ord(ch)] = [int(rows[2 * i:2 * i + 2], 16) for i in range(7)]
    return table


def palette(L):
    """the default class colours, uint8 [L, 3]: class i takes place ((2j + 1) * 768) // L, j = (i * stride) % L, on the
    wheel of 1536 fully saturated colours (red -> yellow -> green -> cyan -> blue -> magenta -> red); stride is the least
    number >= 0.38 L that is coprime to L, so neighbouring classes lie far apart.  The places are distinct for L <= 768 and
    none is 0 or 1535, the two reds -- no class colour equals the default ``kpt_color``."""
    L = int(L)
    if not 1 <= L <= 768:
        raise ValueError('palette: %d classes (1 .. 768)' % L)
    stride = max(1, (38 * L + 99) // 100)
    while np.gcd(stride, L) != 1:
        stride += 1
    out = np.zeros((L, 3), dtype=np.uint8)
    for i in range(L):
        seg, f = divmod(((2 * ((i * stride) % L) + 1) * 768) // L, 256)
        out[i] = [(255, f, 0), (255 - f, 255, 0), (0, 255, f), (0, 255 - f, 255), (f, 0, 255), (255, 0, 255 - f)][seg]
    return out


class Style(object):
    """the validated settings of a picture and the tables derived from the class names"""

    def __init__(self, class_names, landmark_ranges=None, score_thr=0.3, thickness=2, radius=2, contour=False, line_width=1,
                 font_scale=1, kpt_color=KPT_COLOR, colors=None):
        self.names = [n.encode('utf-8') if isinstance(n, str) else bytes(n) for n in class_names]
        self.L = L = len(self.names)
        if not 1 <= L <= 64:
            raise ValueError('%d class names (1 .. 64)' % L)
        if max(len(n) for n in self.names) > MAX_NAME_BYTES:
            raise ValueError('a class name is at most %d bytes' % MAX_NAME_BYTES)
        for what, value, hi in (('thickness', thickness, 64), ('radius', radius, 64), ('line_width', line_width, 16),
                                ('font_scale', font_scale, 8)):
            if int(value) != value or not 1 <= value <= hi:
                raise ValueError('%s is an integer in 1 .. %d, got %r' % (what, hi, value))
        self.score_thr = np.float32(score_thr)
        self.thickness, self.radius, self.line_width, self.font_scale = int(thickness), int(radius), int(line_width), int(font_scale)
        self.contour = bool(contour)
        self.colors = palette(L) if colors is None else np.ascontiguousarray(colors, dtype=np.uint8).reshape(L, 3)
        self.kpt_color = None if kpt_color is None else tuple(int(c) & 255 for c in kpt_color)
        self.ranges = None
        if landmark_ranges is not None:
            self.ranges = np.ascontiguousarray(landmark_ranges, dtype=np.int32).reshape(L, 2)
        self.glyphs = glyph_table()

    def range_of(self, label, K):
        if self.ranges is None:
            return 0, K
        a, b = int(self.ranges[label, 0]), int(self.ranges[label, 1])
        return min(max(a, 0), K), min(max(b, 0), K)


def default_ranges(L, K):
    """DeepFashion2's per-category landmark ranges when (L, K) is that scheme's (13, 294), else None: all K landmarks"""
    from .evaluation import landmark_meta
    ranges = landmark_meta()['landmark_ranges']
    return ranges if (len(ranges) == L and K == 294) else None


def row_count(block):
    """rows in use of one image's [M, 7 + 3K] block: column 6 of row 0, as ``decode.unpack_results`` reads it, cut to [0, M]"""
    c = float(block[0, 6])
    return 0 if not c >= 0 else int(min(c, block.shape[0]))


def _coord(v):
    """float32 value(s) -> rint, clamped, int64 (callers test finiteness first)"""
    return np.clip(np.rint(np.asarray(v, dtype=np.float32)), COORD_MIN, COORD_MAX).astype(np.int64)


def score_digits(score):
    """the three digits q of ``d.dd``"""
    p = np.rint(np.float64(np.float32(score)) * 100.0)
    return int(min(max(p, 0.0), 999.0))


def label_text(name, score):
    q = score_digits(score)
    return name + b'|' + ('%d.%02d' % (q // 100, q % 100)).encode('ascii')


def _capsule_mask(xs, ys, px, py, qx, qy, R2):
    """pixels xs [w], ys [h] (int64) inside the capsule around P -> Q -> bool [h, w]"""
    X, Y = 2 * xs[None, :], 2 * ys[:, None]
    dx, dy = 2 * (qx - px), 2 * (qy - py)
    vx, vy = X - 2 * px, Y - 2 * py
    dot, dd = vx * dx + vy * dy, dx * dx + dy * dy
    wx, wy = X - 2 * qx, Y - 2 * qy
    cross = vx * dy - vy * dx
    return np.where(dot <= 0, vx * vx + vy * vy <= R2, np.where(dot >= dd, wx * wx + wy * wy <= R2, cross * cross <= R2 * dd))


def _window(lo_x, lo_y, hi_x, hi_y, W, H):
    """the inclusive rectangle cut to the image -> (x0, y0, x1, y1) or None"""
    x0, y0, x1, y1 = max(lo_x, 0), max(lo_y, 0), min(hi_x, W - 1), min(hi_y, H - 1)
    return None if (x1 < x0 or y1 < y0) else (x0, y0, x1, y1)


def draw_restatement(image, rows, count, class_names, landmark_ranges=None, score_thr=0.3, thickness=2, radius=2,
                     contour=False, line_width=1, font_scale=1, kpt_color=KPT_COLOR, colors=None, style=None):
    """The picture (see the module's docstring) -> a new uint8 [H, W, 3] array.  Primitives are painted in (row, layer)
    order, each over what is there: the greatest covering (r, layer) stays.  ``style``: a prepared ``Style`` instead of the
    keywords."""
    st = style or Style(class_names, landmark_ranges, score_thr, thickness, radius, contour, line_width, font_scale, kpt_color,
                        colors)
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise TypeError('an image is a uint8 H x W x 3 array')
    H, W = image.shape[:2]
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError('image of %d x %d (sides 1 .. %d)' % (H, W, MAX_SIDE))
    rows = np.asarray(rows, dtype=np.float32)
    M, K = rows.shape[0], (rows.shape[1] - 7) // 3
    if rows.ndim != 2 or rows.shape[1] != 7 + 3 * K or K < 1:
        raise ValueError('rows of 7 + 3K floats, K >= 1')
    out = image.copy()
    t, rad, s, R2 = st.thickness, st.radius, st.font_scale, st.line_width ** 2
    pad = (st.line_width + 1) // 2
    for r in range(min(max(int(count), 0), M)):
        row = rows[r]
        lab = row[5]
        if not (row[4] > st.score_thr and lab == np.floor(lab) and 0 <= lab < st.L and np.isfinite(row[:4]).all()):
            continue
        lab = int(lab)
        colour = st.colors[lab]
        x0, y0, x1, y1 = (int(c) for c in _coord(row[:4]))
        # 0: the box
        if x1 >= x0 and y1 >= y0:
            win = _window(x0, y0, x1, y1, W, H)
            if win is not None:
                xs, ys = np.arange(win[0], win[2] + 1), np.arange(win[1], win[3] + 1)
                ring = ((xs < x0 + t) | (xs > x1 - t))[None, :] | ((ys < y0 + t) | (ys > y1 - t))[:, None]
                out[win[1]:win[3] + 1, win[0]:win[2] + 1][ring] = colour
        a, b = st.range_of(lab, K)
        pts = row[7 + 3 * a:7 + 3 * b].reshape(-1, 3)
        ok = (pts[:, 2] > 0) & np.isfinite(pts[:, 0]) & np.isfinite(pts[:, 1])
        cx, cy = _coord(np.where(ok, pts[:, 0], 0)), _coord(np.where(ok, pts[:, 1], 0))
        # 1: the contour
        if st.contour:
            for k in np.nonzero(ok[:-1] & ok[1:])[0]:
                px, py, qx, qy = int(cx[k]), int(cy[k]), int(cx[k + 1]), int(cy[k + 1])
                win = _window(min(px, qx) - pad, min(py, qy) - pad, max(px, qx) + pad, max(py, qy) + pad, W, H)
                if win is not None:
                    xs, ys = np.arange(win[0], win[2] + 1, dtype=np.int64), np.arange(win[1], win[3] + 1, dtype=np.int64)
                    out[win[1]:win[3] + 1, win[0]:win[2] + 1][_capsule_mask(xs, ys, px, py, qx, qy, R2)] = colour
        # 2: the landmarks
        dot_colour = colour if st.kpt_color is None else st.kpt_color
        for k in np.nonzero(ok)[0]:
            px, py = int(cx[k]), int(cy[k])
            win = _window(px - rad, py - rad, px + rad, py + rad, W, H)
            if win is not None:
                xs, ys = np.arange(win[0], win[2] + 1, dtype=np.int64), np.arange(win[1], win[3] + 1, dtype=np.int64)
                disc = (xs[None, :] - px) ** 2 + (ys[:, None] - py) ** 2 <= rad * rad
                out[win[1]:win[3] + 1, win[0]:win[2] + 1][disc] = dot_colour
        # 3: the label
        text = label_text(st.names[lab], row[4])
        top = y0 - 9 * s
        if top < 0:
            top = y0
        win = _window(x0, top, x0 + (6 * len(text) + 1) * s - 1, top + 9 * s - 1, W, H)
        if win is not None:
            ink = (0, 0, 0) if 299 * int(colour[0]) + 587 * int(colour[1]) + 114 * int(colour[2]) >= 128000 else (255, 255, 255)
            gx, gy = (np.arange(win[0], win[2] + 1) - x0) // s, (np.arange(win[1], win[3] + 1) - top) // s
            gi, col = (gx - 1) // 6, (gx - 1) % 6                       # (gx = 0: glyph -1, never inked)
            masks = st.glyphs[np.frombuffer(text, dtype=np.uint8)]        # [n, 7]
            inked_x = (gx >= 1) & (col < 5)
            line_ok = (gy >= 1) & (gy <= 7)
            bits = (masks[np.clip(gi, 0, len(text) - 1)][:, np.clip(gy - 1, 0, 6)].T >> (4 - np.clip(col, 0, 4))[None, :]) & 1
            fg = (bits == 1) & inked_x[None, :] & line_ok[:, None]
            view = out[win[1]:win[3] + 1, win[0]:win[2] + 1]
            view[:] = colour
            view[fg] = ink
    return out


def result_rows(result):
    """what ``inference_detector`` returns for one image -- ``(boxes per class, scores, landmarks per class)`` or the 1-tuple of
    an empty image -> (rows float32 [max(n, 1), 7 + 3K], n) in ``np.vstack`` order of the classes (K = 1 for the empty one)"""
    if len(result) == 1 or sum(len(b) for b in result[0]) == 0:
        return np.zeros((1, 10), dtype=np.float32), 0
    boxes, kpts = result[0], result[2]
    det = np.vstack(boxes).astype(np.float32)
    labels = np.concatenate([np.full(len(b), c, dtype=np.float32) for c, b in enumerate(boxes)])
    kp = np.vstack([np.asarray(k).reshape(len(b), -1) for b, k in zip(boxes, kpts) if len(b)]).astype(np.float32)
    n = det.shape[0]
    rows = np.concatenate([det[:, :5], labels[:, None], np.full((n, 1), n, dtype=np.float32), kp], axis=1)
    return np.ascontiguousarray(rows, dtype=np.float32), n


def stack_result_rows(results, M=None):
    """several images' results -> one block [n, M, 7 + 3K] (M: the largest count, at least 1; unused rows are zero) with the
    counts in column 6"""
    packed = [result_rows(r) for r in results]
    width = max(p[0].shape[1] for p in packed)
    M = max([M or 1] + [p[1] for p in packed])
    block = np.zeros((len(packed), M, width), dtype=np.float32)
    for i, (rows, n) in enumerate(packed):
        if n:
            block[i, :n, :rows.shape[1]] = rows
        block[i, :, 6] = n
    return block


def denormalize(chw, mean, std, to_rgb=True):
    """a normalised [3, H, W] float image -> uint8 [H, W, 3] RGB (mmcv's ``tensor2imgs`` for one image)"""
    img = np.asarray(chw, dtype=np.float32).transpose(1, 2, 0) * np.asarray(std, np.float32) + np.asarray(mean, np.float32)
    if not to_rgb:
        img = img[..., ::-1]
    return np.ascontiguousarray(np.clip(np.rint(img), 0, 255).astype(np.uint8))


def device_available():
    """a GPU and the built library: the condition under which ``show_result`` draws with the kernel"""
    import torch
    from . import _lib
    return torch.cuda.is_available() and os.path.exists(_lib.LIB_PATH)


class DeviceDrawer(object):
    """``kgdet_draw_detections`` with its tables in device memory (uploaded once).  ``drawer(images, rows)``: ``images`` a list
    of uint8 [H, W, 3] host arrays or tensors (host or device), ``rows`` their [n, M, 7 + 3K] block, a device tensor or numpy
    (uploaded) -> the drawn images as device tensors, views of one buffer; ``to_host=True``: numpy arrays, through one
    page-locked download.  ``blocks``: the row block of each image when it is not its place in the list.  Groups of
    ``MAX_IMAGES`` images share a launch."""

    def __init__(self, class_names, landmark_ranges=None, score_thr=0.3, thickness=2, radius=2, contour=False, line_width=1,
                 font_scale=1, kpt_color=KPT_COLOR, colors=None, device=None):
        import torch
        self.style = st = Style(class_names, landmark_ranges, score_thr, thickness, radius, contour, line_width, font_scale,
                                kpt_color, colors)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        offsets = np.concatenate([[0], np.cumsum([len(n) for n in st.names])]).astype(np.int32)
        names = np.frombuffer(b''.join(st.names) + b'\0', dtype=np.uint8).copy()        # (never empty)

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.colors, self.names, self.name_off, self.glyphs = up(st.colors), up(names), up(offsets), up(st.glyphs)
        self.name_total = int(offsets[-1])
        self.ranges = None if st.ranges is None else up(st.ranges)
        self.kpt = -1 if st.kpt_color is None else (st.kpt_color[0] << 16 | st.kpt_color[1] << 8 | st.kpt_color[2])

    def __call__(self, images, rows, to_host=False, blocks=None):
        import torch
        n = len(images)
        if torch.is_tensor(rows):
            rows = rows.to(self.device, torch.float32).contiguous()
        else:
            rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(self.device)
        if rows.dim() != 3:
            raise ValueError('rows is a [n, M, 7 + 3K] block')
        blocks = list(range(n)) if blocks is None else [int(b) for b in blocks]
        if len(blocks) != n or any(not 0 <= b < rows.shape[0] for b in blocks):
            raise ValueError('one row block in [0, %d) per image' % rows.shape[0])
        if n == 0:
            return []
        shapes, at, total = [], [], 0
        for img in images:
            if tuple(img.shape[2:]) != (3,) or len(img.shape) != 3 or str(img.dtype).split('.')[-1] != 'uint8':
                raise TypeError('an image is a uint8 H x W x 3 array or tensor')
            shapes.append((int(img.shape[0]), int(img.shape[1])))
            at.append(total)
            total += (3 * shapes[-1][0] * shapes[-1][1] + 255) // 256 * 256
        src = torch.empty(total, dtype=torch.uint8, device=self.device)
        on_device = [torch.is_tensor(img) and img.is_cuda for img in images]
        staged = None if all(on_device) else torch.empty(total, dtype=torch.uint8).pin_memory()
        for img, (H, W), off, there in zip(images, shapes, at, on_device):
            size = 3 * H * W
            if there:
                src[off:off + size].view(H, W, 3).copy_(img)
                continue
            staged[off:off + size].view(H, W, 3).copy_(img if torch.is_tensor(img) else torch.from_numpy(np.ascontiguousarray(img)))
            if any(on_device):
                src[off:off + size].copy_(staged[off:off + size], non_blocking=True)
        if not any(on_device):          # host images only: one upload from page-locked memory
            src.copy_(staged, non_blocking=True)
        dst = torch.empty(total, dtype=torch.uint8, device=self.device)
        self.launch(src, dst, at, shapes, rows, blocks)
        if not to_host:
            return [dst[off:off + 3 * H * W].view(H, W, 3) for (H, W), off in zip(shapes, at)]
        host = torch.empty(total, dtype=torch.uint8).pin_memory()
        host.copy_(dst, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        flat = host.numpy()
        return [flat[off:off + 3 * H * W].reshape(H, W, 3) for (H, W), off in zip(shapes, at)]

    def launch(self, src, dst, offsets, shapes, rows, blocks):
        """the launches alone: image i of ``shapes`` [(H, W)] lies ``offsets[i]`` bytes into the flat uint8 device buffer
        ``src`` and is drawn at the same offset of ``dst`` from block ``blocks[i]`` of the device tensor ``rows``"""
        import ctypes
        import torch
        from . import _lib
        st, lib, p = self.style, _lib.lib(), _lib.ptr
        i32, i64 = ctypes.c_int32, ctypes.c_int64
        n = len(shapes)
        with torch.cuda.device(self.device):
            for g in range(0, n, MAX_IMAGES):
                m = min(MAX_IMAGES, n - g)
                table = (i64 * (4 * m))(*[v for i in range(g, g + m) for v in (offsets[i], offsets[i], shapes[i][0], shapes[i][1])])
                blk = (i32 * m)(*blocks[g:g + m])
                rc = lib.kgdet_draw_detections(
                    p(src), i64(src.numel()), p(dst), i64(dst.numel()), table, blk, i32(m), p(rows), i64(rows.shape[0]),
                    i32(rows.shape[1]), i32(rows.shape[2]), p(self.colors), i32(st.L), p(self.names), p(self.name_off),
                    i32(self.name_total), p(self.ranges), p(self.glyphs), ctypes.c_float(float(st.score_thr)), i32(st.thickness),
                    i32(st.radius), i32(int(st.contour)), i32(st.line_width), i32(st.font_scale), i32(self.kpt),
                    _lib.current_stream())
                _lib.check(rc, 'kgdet_draw_detections')


def save_image(array, path, ext=None):
    """one picture through PIL, by ``ext`` or the path's extension: JPEG at quality 90, else what PIL makes of it (PNG)"""
    from PIL import Image
    ext = (ext or os.path.splitext(path)[1]).lower()
    if ext in ('.jpg', '.jpeg'):
        Image.fromarray(array).save(path, format='JPEG', quality=90)
    elif ext == '.png':
        Image.fromarray(array).save(path, format='PNG')
    else:
        Image.fromarray(array).save(path)


def show_result(img, result, class_names, score_thr=0.3, wait_time=0, show=False, out_file=None, **style):
    """``mmdet.apis.show_result`` for a KGDet result, landmarks included.  ``img``: a path or a uint8 RGB array; ``result``:
    what ``inference_detector`` returns for it.  Drawn by ``kgdet_draw_detections`` when a GPU and the library are there,
    else by ``draw_restatement`` -- the same bits.  ``style``: ``thickness``, ``radius``, ``contour``, ``line_width``,
    ``font_scale``, ``kpt_color``, ``colors``, ``landmark_ranges`` (default: DeepFashion2's for its 13 classes and 294
    landmarks).  Returns the array when ``out_file`` is None, else writes that file (PIL, by its extension -- a ``.jpg`` too:
    PIL's encoder at quality 90; for the bytes of the GPU encoder pass the returned array to ``jpeg.encode_jpeg``).
    ``show=True`` raises: there is no window system (``wait_time`` is the reference's and unused)."""
    if show:
        raise NotImplementedError('show=True needs a window system; pass out_file or take the returned array')
    if isinstance(img, str):
        from PIL import Image
        with Image.open(img) as im:
            img = np.array(im.convert('RGB'))
    img = np.ascontiguousarray(img)
    rows, count = result_rows(result)
    if 'landmark_ranges' not in style:
        style['landmark_ranges'] = default_ranges(len(class_names), (rows.shape[1] - 7) // 3)
    if device_available():
        drawn = DeviceDrawer(class_names, score_thr=score_thr, **style)([img], rows[None], to_host=True)[0].copy()
    else:
        drawn = draw_restatement(img, rows, count, class_names, score_thr=score_thr, **style)
    if out_file is None:
        return drawn
    save_image(drawn, out_file)
    return None


class PictureWriter(object):
    """finished pictures -> files of ``show_dir``, encoded by a bounded pool of ``workers`` threads (at least 1, at most 16):
    ``put`` (an array, encoded by the thread) and ``put_bytes`` (a file's bytes, only written by it) block while 2 x workers
    pictures wait, and re-raise a writer's exception; ``close()`` ends the threads -- after a
    failure (``failed=True``) without waiting for queued pictures, otherwise after the last one, re-raising what it met."""

    def __init__(self, show_dir, workers=1, ext='.jpg'):
        from concurrent.futures import ThreadPoolExecutor
        if ext.lower() not in ('.jpg', '.jpeg', '.png'):
            raise ValueError('show_ext is .jpg or .png, got %r' % (ext,))
        self.dir, self.ext = show_dir, ext
        self.workers = min(max(int(workers), 1), 16)
        os.makedirs(show_dir, exist_ok=True)
        self.pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix='kgdet-show-writer')
        self.pending = deque()

    def _write(self, array, name):
        save_image(array, os.path.join(self.dir, name + self.ext), self.ext)

    def _write_bytes(self, data, name):
        with open(os.path.join(self.dir, name + self.ext), 'wb') as f:
            f.write(data)

    def put(self, array, name):
        while len(self.pending) >= 2 * self.workers:
            self.pending.popleft().result()
        self.pending.append(self.pool.submit(self._write, array, name))

    def put_bytes(self, data, name):
        """a finished file (``jpeg.DeviceJpegEncoder``'s bytes): the thread only writes it; same queue and bounds as ``put``"""
        while len(self.pending) >= 2 * self.workers:
            self.pending.popleft().result()
        self.pending.append(self.pool.submit(self._write_bytes, data, name))

    def close(self, failed=False):
        try:
            while self.pending and not failed:
                self.pending.popleft().result()
        finally:
            self.pending.clear()
            self.pool.shutdown(wait=True, cancel_futures=True)
