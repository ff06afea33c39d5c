"""Baseline JPEG files of the drawn pictures made on the GPU: ``jpeg_restatement``, ``DeviceJpegEncoder``, ``encode_jpeg``.

``visualize.DeviceDrawer`` leaves a finished picture in device memory; ``kgdet_jpeg_encode`` / ``kgdet_jpeg_write``
(csrc/jpeg.hip) turn that buffer into the bytes of the ``.jpg`` file, so that only compressed bytes come down.  The file is
DEFINED here, once, by ``jpeg_restatement`` (numpy and Python integers); it is the CPU fallback of ``encode_jpeg`` and the
yardstick of the kernels, which are held to it byte for byte.  The bytes of cv2's, mmcv's, PIL's or libjpeg's own encoders are
unpinned (tests/test_jpeg_refs.py holds the definition to a float64 reference, to a parser written for the test and to PIL's
decoder).

The file
--------
Baseline sequential JFIF (``SOF0``, 8 bit), components Y / Cb / Cr sampled 2x2 / 1x1 / 1x1 (4:2:0; an MCU is 16 x 16 pixels,
its blocks in the order Y00 Y01 Y10 Y11 Cb Cr), one interleaved scan, no restart intervals.  Markers: ``SOI``, ``APP0`` (JFIF
1.01, no units, density 1:1, no thumbnail), ``DQT`` luminance (table 0), ``DQT`` chrominance (table 1), ``SOF0``, ``DHT`` DC
luminance, AC luminance, DC chrominance, AC chrominance, ``SOS``, data, ``EOI``: ``HEADER_BYTES`` = 623 bytes in front of the
data, of which only the four size bytes of ``SOF0`` depend on the image.

Tables: the quantisation tables of ITU T.81 Annex K.1 scaled by the IJG rule -- s = 5000 // q for q < 50, else 200 - 2q; entry
= clamp((base * s + 50) // 100, 1, 255) -- for ``quality`` q in 1 .. 100, and the four typical Huffman tables of Annex K.3.

Pixels to coefficients, all in integers (image uint8 [H, W, 3] RGB, 1 <= H, W <= 8192):

1. Edges: column W - 1 and row H - 1 are replicated up to whole MCUs.
2. Colour (JFIF / BT.601 full range, coefficients rint(65536 c), ``>>`` is the arithmetic shift = floor), each sample with FOUR
   fraction bits and one rounding, level-shifted (128 * 16 = 2048):
   Y  = ((19595 R + 38470 G + 7471 B + 2048) >> 12) - 2048;
   Cb = (-11058 SR - 21710 SG + 32768 SB + 8192) >> 14, Cr = (32768 SR - 27439 SG - 5329 SB + 8192) >> 14
   with SR, SG, SB the sums over the 2 x 2 pixels of the chroma sample: the mean of the four chroma values, rounded once.
   (Samples rounded to whole grey levels first would be off by up to 1/2 each, all one way in a flat region: 4 in the DC
   coefficient, more than a quantisation step at quality 90.)  |sample| <= 2048.
3. DCT of each 8 x 8 block, rows then columns, with the matrix D[u][x] = rint(8192 c(u) cos((2x + 1) u pi / 16)), c(0) =
   sqrt(1/8), c(u) = 1/2: up to sign its entries are ``DCT_CONST`` = 2896 (u = 0) and 4017, 3784, 3406, 2896, 2276, 1567, 799
   (cos(k pi / 16) / 2, k = 1 .. 7).  Rows: P = (X D^T + 1024) >> 11 (six fraction bits); columns: C = (D P + 32768) >> 16, the
   coefficient times 8.  |X D^T| <= 8 * 4017 * 2048 < 2^26, |P| < 2^15 and |D P| < 8 * 4017 * 2^15 < 2^30: int32 holds everything.
4. Quantisation, half away from zero: level = sign(C) * ((|C| + 4 q) // (8 q)), q the table's entry.
5. Zigzag order.

``ERROR_BOUND`` E, the distance of C / 8 from the exact (float64) coefficient of the same pixels, from the expressions above:
a sample (luma, or the chroma mean) is off by at most 1/32 (the one rounding) + 3 * 255 / 2^17 (three matrix entries, each
within 2^-17) = eps; the two-dimensional DCT is orthonormal with basis sums of at most 8, so the samples cost 8 eps = 0.297.
The row pass adds 8 * 128 / 2 / 8192 (matrix rounding against |x| <= 128) + 2^-7 (its shift) = 0.0704 per entry, which the
column pass carries with gain sum |D[u]| / 8192 <= 2.83 (u = 0) to 0.199; the column pass adds 8 * 363 / 2 / 8192 = 0.178
(matrix rounding against |P| <= 128 * 2.83 < 363) + 1/16 (its shift).  E = 0.297 + 0.199 + 0.178 + 0.0625 < 0.74: below one
quantisation step at every quality, so a level is never off by more than 1.

Entropy coding: per component the DC difference to the previous block of that component in scan order (0 before the first),
coded by its size category and the magnitude bits of F.1.2 (a negative value v as v - 1 in ``size`` bits); AC as (run, size)
symbols with ``ZRL`` (0xF0) for every 16 zeros before a coefficient and ``EOB`` (0x00) when the block ends in zeros.  The bit
stream is padded with 1-bits to a whole byte, and every 0xFF data byte -- one the padding made included -- is followed by 0x00.
"""
import os

import numpy as np

MAX_SIDE = 8192
MAX_IMAGES = 32             # KGDET_JPEG_MAX_IMAGES: images of one call
HEADER_BYTES = 623
RANGE_BYTES = 4096          # KGDET_JPEG_RANGE_BYTES: bytes of the unstuffed stream one workgroup of the pack kernel owns

BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
    + [99] * 32, dtype=np.int64)
# natural index of the k-th coefficient in zigzag order
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63],
    dtype=np.int64)

DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUMA_VALS = list(bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546'
    '4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7'
    'b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa'))
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = list(bytes.fromhex(
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445'
    '464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5'
    'b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa'))

DCT_CONST = (2896, 4017, 3784, 3406, 2896, 2276, 1567, 799)         # [0]: u = 0; [k]: cos(k pi / 16) / 2, both times 8192
ERROR_BOUND = 8 * (1 / 32.0 + 3 * 255 / 2.0 ** 17) + 2.83 * (8 * 128 / 2.0 / 8192 + 2.0 ** -7) + 8 * 363 / 2.0 / 8192 + 1 / 16.0


def dct_matrix():
    """D int64 [8, 8] of step 3, from ``DCT_CONST`` by the cosine's symmetries"""
    D = np.zeros((8, 8), dtype=np.int64)
    for u in range(8):
        for x in range(8):
            if u == 0:
                D[u, x] = DCT_CONST[0]
                continue
            j, sign = ((2 * x + 1) * u) % 32, 1
            if j > 16:
                j = 32 - j
            if j > 8:
                j, sign = 16 - j, -1
            D[u, x] = 0 if j == 8 else sign * DCT_CONST[j]
    return D


def _check_quality(quality):
    if int(quality) != quality or not 1 <= quality <= 100:
        raise ValueError('quality is an integer in 1 .. 100, got %r' % (quality,))
    return int(quality)


def quant_tables(quality=90):
    """int64 [2, 64]: the luminance and the chrominance table at ``quality``, in natural (row-major) order"""
    q = _check_quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((base * s + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA)])


def huffman_codes(bits, vals):
    """Annex C: a table's (code, length) per symbol -> int64 [256, 2], length 0 for a symbol the table lacks"""
    out = np.zeros((256, 2), dtype=np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def _check_image(image):
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise TypeError('an image is a uint8 H x W x 3 array')
    H, W = image.shape[:2]
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError('image of %d x %d (sides 1 .. %d)' % (H, W, MAX_SIDE))
    return image


def sample_planes(image):
    """steps 1 and 2 -> (Y int64 [16 mh, 16 mw], Cb, Cr int64 [8 mh, 8 mw]), level-shifted, times 16"""
    image = _check_image(image)
    H, W = image.shape[:2]
    mh, mw = (H + 15) // 16, (W + 15) // 16
    px = np.pad(image.astype(np.int64), ((0, 16 * mh - H), (0, 16 * mw - W), (0, 0)), mode='edge')
    R, G, B = px[..., 0], px[..., 1], px[..., 2]
    Y = ((19595 * R + 38470 * G + 7471 * B + 2048) >> 12) - 2048
    S = px.reshape(8 * mh, 2, 8 * mw, 2, 3).sum(axis=(1, 3))
    Cb = (-11058 * S[..., 0] - 21710 * S[..., 1] + 32768 * S[..., 2] + 8192) >> 14
    Cr = (32768 * S[..., 0] - 27439 * S[..., 1] - 5329 * S[..., 2] + 8192) >> 14
    return Y, Cb, Cr


def _blocks(plane):
    """[8 a, 8 b] -> [a, b, 8, 8]"""
    a, b = plane.shape[0] // 8, plane.shape[1] // 8
    return plane.reshape(a, 8, b, 8).transpose(0, 2, 1, 3)


def quantized_blocks(image, quality=90):
    """steps 1 .. 4 -> (Y int64 [2 mh, 2 mw, 8, 8], Cb, Cr int64 [mh, mw, 8, 8]): the quantised levels in natural order"""
    Q = quant_tables(quality)
    D = dct_matrix()
    out = []
    for plane, q in zip(sample_planes(image), (Q[0], Q[1], Q[1])):
        X = _blocks(plane)
        P = (np.einsum('abyx,ux->abyu', X, D) + 1024) >> 11
        C = (np.einsum('vy,abyu->abvu', D, P) + 32768) >> 16
        q = q.reshape(8, 8)
        out.append(np.sign(C) * ((np.abs(C) + 4 * q) // (8 * q)))
    return tuple(out)


def header(H, W, quality=90):
    """the ``HEADER_BYTES`` bytes from ``SOI`` to the end of ``SOS``"""
    Q = quant_tables(quality)
    out = bytearray(b'\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for t in range(2):
        out += b'\xff\xdb\x00\x43' + bytes([t]) + bytes(int(v) for v in Q[t][ZIGZAG])
    out += b'\xff\xc0\x00\x11\x08' + bytes([H >> 8, H & 255, W >> 8, W & 255]) + b'\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01'
    for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                              (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        n = 19 + len(vals)
        out += b'\xff\xc4' + bytes([n >> 8, n & 255, tc_th]) + bytes(bits) + bytes(vals)
    out += b'\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00'
    assert len(out) == HEADER_BYTES
    return bytes(out)


class _Bits(object):
    def __init__(self):
        self.acc, self.n, self.total, self.out = 0, 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        self.total += length
        if self.n >= 256:
            keep = self.n & 7
            self.out += (self.acc >> keep).to_bytes((self.n - keep) // 8, 'big')
            self.acc &= (1 << keep) - 1
            self.n = keep

    def finish(self):
        pad = -self.n & 7
        acc, n = (self.acc << pad) | ((1 << pad) - 1), self.n + pad
        return bytes(self.out + acc.to_bytes(n // 8, 'big'))


def _size(v):
    return int(abs(int(v))).bit_length()


def entropy_code(Y, Cb, Cr):
    """the scan of the quantised blocks -> (the unstuffed, padded stream, its bits before the padding)"""
    dc = (huffman_codes(DC_LUMA_BITS, DC_VALS), huffman_codes(DC_CHROMA_BITS, DC_VALS))
    ac = (huffman_codes(AC_LUMA_BITS, AC_LUMA_VALS), huffman_codes(AC_CHROMA_BITS, AC_CHROMA_VALS))
    mh, mw = Cb.shape[:2]
    zz = [np.ascontiguousarray(p.reshape(p.shape[0], p.shape[1], 64)[..., ZIGZAG]) for p in (Y, Cb, Cr)]
    bits = _Bits()
    pred = [0, 0, 0]
    for my in range(mh):
        for mx in range(mw):
            for comp, t, by, bx in ((0, 0, 2 * my, 2 * mx), (0, 0, 2 * my, 2 * mx + 1), (0, 0, 2 * my + 1, 2 * mx),
                                    (0, 0, 2 * my + 1, 2 * mx + 1), (1, 1, my, mx), (2, 1, my, mx)):
                blk = zz[comp][by, bx]
                diff = int(blk[0]) - pred[comp]
                pred[comp] = int(blk[0])
                s = _size(diff)
                bits.put(int(dc[t][s, 0]), int(dc[t][s, 1]))
                if s:
                    bits.put(diff if diff > 0 else diff - 1 + (1 << s), s)
                last = 0
                for k in np.nonzero(blk[1:])[0] + 1:
                    v, run = int(blk[k]), int(k) - 1 - last
                    last = int(k)
                    while run >= 16:
                        bits.put(int(ac[t][0xF0, 0]), int(ac[t][0xF0, 1]))
                        run -= 16
                    s = _size(v)
                    bits.put(int(ac[t][run << 4 | s, 0]), int(ac[t][run << 4 | s, 1]))
                    bits.put(v if v > 0 else v - 1 + (1 << s), s)
                if last != 63:
                    bits.put(int(ac[t][0, 0]), int(ac[t][0, 1]))
    total = bits.total
    return bits.finish(), total


def jpeg_parts(image, quality=90):
    """the restatement with its intermediate results: dict(bytes, blocks=(Y, Cb, Cr), bits, stream)"""
    image = _check_image(image)
    Y, Cb, Cr = quantized_blocks(image, quality)
    stream, total = entropy_code(Y, Cb, Cr)
    data = header(image.shape[0], image.shape[1], quality) + stream.replace(b'\xff', b'\xff\x00') + b'\xff\xd9'
    return dict(bytes=data, blocks=(Y, Cb, Cr), bits=total, stream=stream)


def jpeg_restatement(image, quality=90):
    """The file (see the module's docstring) of a uint8 [H, W, 3] RGB array -> bytes"""
    return jpeg_parts(image, quality)['bytes']


def device_available():
    """a GPU and the built library: the condition under which ``encode_jpeg`` uses the kernels"""
    import torch
    from . import _lib
    return torch.cuda.is_available() and os.path.exists(_lib.LIB_PATH)


class DeviceJpegEncoder(object):
    """``kgdet_jpeg_encode`` / ``kgdet_jpeg_write`` at one ``quality``.  ``encoder(images)``: ``images`` a list of uint8 [H, W, 3]
    device tensors -> the list of their files as ``bytes``, byte for byte ``jpeg_restatement``'s.  Contiguous views of ONE
    buffer, as ``DeviceDrawer`` returns them, are encoded where they lie; other tensors are gathered into one buffer first.
    Per group of ``MAX_IMAGES`` images: the launches, one read-back of the file lengths (the point where the output must be
    sized), the launch that writes the files and one download of them through page-locked memory.  The quantisation tables
    and the header travel as kernel arguments made from ``quality`` by the library and the Huffman tables are constants of
    the kernels, so the encoder keeps no table of its own on the device: only its workspace, which grows to the largest group
    seen (about 2.7 bytes per byte of pixels)."""

    def __init__(self, quality=90, device=None):
        import torch
        self.quality = _check_quality(quality)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.workspace = None
        self.downloaded = 0                  # bytes of files downloaded so far (tools/time_jpeg.py)

    def __call__(self, images):
        import torch
        images = list(images)
        if not images:
            return []
        for img in images:
            if not (torch.is_tensor(img) and img.is_cuda and img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3):
                raise TypeError('an image is a uint8 H x W x 3 device tensor')
            if not (1 <= img.shape[0] <= MAX_SIDE and 1 <= img.shape[1] <= MAX_SIDE):
                raise ValueError('image of %d x %d (sides 1 .. %d)' % (img.shape[0], img.shape[1], MAX_SIDE))
        shapes = [(int(img.shape[0]), int(img.shape[1])) for img in images]
        store = images[0].untyped_storage()
        if all(img.is_contiguous() and img.untyped_storage().data_ptr() == store.data_ptr() for img in images):
            src = torch.empty(0, dtype=torch.uint8, device=images[0].device).set_(store)
            offsets = [img.data_ptr() - store.data_ptr() for img in images]
        else:
            offsets, total = [], 0
            for H, W in shapes:
                offsets.append(total)
                total += (3 * H * W + 255) // 256 * 256
            src = torch.empty(total, dtype=torch.uint8, device=self.device)
            for img, (H, W), off in zip(images, shapes, offsets):
                src[off:off + 3 * H * W].view(H, W, 3).copy_(img)
        out = []
        with torch.cuda.device(src.device):
            for g in range(0, len(images), MAX_IMAGES):
                out.extend(self.encode(src, offsets[g:g + MAX_IMAGES], shapes[g:g + MAX_IMAGES]))
        return out

    def encode(self, src, offsets, shapes):
        """one group: image i of ``shapes`` [(H, W)] lies ``offsets[i]`` bytes into the flat uint8 device buffer ``src``"""
        import ctypes
        import torch
        from . import _lib
        lib, p, stream = _lib.lib(), _lib.ptr, _lib.current_stream()
        i32, i64 = ctypes.c_int32, ctypes.c_int64
        n, dev = len(shapes), src.device
        place = [0] * n
        table = (i64 * (4 * n))()

        def fill():
            table[:] = [v for i in range(n) for v in (offsets[i], place[i], shapes[i][0], shapes[i][1])]
        fill()
        need = lib.kgdet_jpeg_workspace_bytes(table, i32(n))
        if need == 0:
            _lib.check(_lib.KGDET_E_SHAPE, 'kgdet_jpeg_workspace_bytes')
        if self.workspace is None or self.workspace.numel() < need or self.workspace.device != dev:
            self.workspace = None
            self.workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        ws = self.workspace
        lengths = torch.empty(n, dtype=torch.int64, device=dev)
        _lib.check(lib.kgdet_jpeg_encode(p(src), i64(src.numel()), table, i32(n), i32(self.quality), p(ws),
                                         ctypes.c_size_t(ws.numel()), p(lengths), stream), 'kgdet_jpeg_encode')
        pinned = torch.empty(n, dtype=torch.int64).pin_memory()
        pinned.copy_(lengths, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()            # the one read-back: the output is sized here
        sizes = [int(v) for v in pinned.tolist()]
        total = 0
        for i, size in enumerate(sizes):
            place[i] = total
            total += (size + 15) // 16 * 16
        fill()
        files = torch.empty(total + 16 * ((4 * n + 15) // 16), dtype=torch.uint8, device=dev)     # the files, then the status words
        status = files[total:total + 4 * n].view(torch.int32)
        capacity = (i64 * n)(*sizes)
        _lib.check(lib.kgdet_jpeg_write(table, i32(n), i32(self.quality), p(ws), ctypes.c_size_t(ws.numel()), capacity, p(files),
                                        i64(total), p(status), stream), 'kgdet_jpeg_write')
        host = torch.empty(files.numel(), dtype=torch.uint8).pin_memory()
        host.copy_(files, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        flat = host.numpy()
        if flat[total:total + 4 * n].view(np.int32).any():
            raise RuntimeError('kgdet_jpeg_write: a file did not fit the length kgdet_jpeg_encode reported')
        self.downloaded += total
        return [flat[at:at + size].tobytes() for at, size in zip(place, sizes)]


def encode_jpeg(image, quality=90):
    """the ``.jpg`` file of a uint8 [H, W, 3] RGB array (or device tensor) as ``bytes``: by ``DeviceJpegEncoder`` when a GPU and
    the library are there, else by ``jpeg_restatement`` -- the same bytes"""
    import torch
    if device_available():
        if not torch.is_tensor(image):
            image = torch.from_numpy(np.array(_check_image(image)))
        return DeviceJpegEncoder(quality, device=image.device if image.is_cuda else None)([image.cuda()])[0]
    if torch.is_tensor(image):
        image = image.cpu().numpy()
    return jpeg_restatement(image, quality)
