"""Baseline JPEG on the GPU, both ways.  Files of the drawn pictures: ``jpeg_restatement``, ``DeviceJpegEncoder``, ``encode_jpeg``
(this docstring).  Pictures of JPEG files, for the loader and the test loop: ``parse_header``, ``decode_restatement`` (the
definition, in its docstring), ``DeviceJpegDecoder``, ``decode_jpeg``, ``DeviceDecodeRoute`` (the second half of the module).

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


# ---- decoding ----------------------------------------------------------------------------------------------------------------
DECODE_MAX_IMAGES = 32      # KGDET_JPEG_DECODE_MAX_IMAGES: images of one call
DECODE_SUBSEQ_BITS = 512    # KGDET_JPEG_DECODE_SUBSEQ_BITS: bits of the un-stuffed stream one lane of the Huffman kernel owns
DECODE_CHUNK_LANES = 1024   # KGDET_JPEG_DECODE_CHUNK_LANES: subsequences a workgroup brings to their fixpoint together
DECODE_TABLE_BYTES = 1024   # KGDET_JPEG_DECODE_TABLE_BYTES: the table block of one image inside the source buffer
MODE_GREY, MODE_444, MODE_420 = 0, 1, 2         # KGDET_JPEG_DECODE_GREY / _444 / _420
MODE_422 = 3                                    # KGDET_JPEG_DECODE_422: the ``camera`` entry points only
BLOCKS_PER_MCU = (1, 3, 6, 4)
SLOT_COMPONENT = ((0,), (0, 1, 2), (0, 0, 0, 0, 1, 2), (0, 0, 1, 2))     # the component of each block slot of the MCU, by mode
MAX_RESTART_INTERVAL = 65535
INVALID = (-1, -1, -1)      # the state of a parse that met an unmatched code or left the block: equal to no valid state

IDCT_CONST = dict(c0_298=2446, c0_390=3196, c0_541=4433, c0_765=6270, c0_899=7373, c1_175=9633, c1_501=12299, c1_847=15137,
                  c1_961=16069, c2_053=16819, c2_562=20995, c3_072=25172)


def _kraft_ok(bits):
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code > (1 << length):
            return False
        code <<= 1
    return True


def parse_header(data, camera=False):
    """Walk the segments of a JPEG file up to the end of ``SOS`` (segment lengths only; no entropy byte is touched) -> the frame
    description the decoder needs, or a REASON STRING (in the style of ``head_loss.why_not``) for a file it does not take.

    Taken: ``SOF0`` with 8-bit samples, 1 <= H, W <= 8192; one interleaved scan (Ss = 0, Se = 63, Ah = Al = 0) of three components
    sampled 2x2 / 1x1 / 1x1 or 1x1 / 1x1 / 1x1 -- YCbCr: a JFIF ``APP0`` or the ids 1, 2, 3 -- or of one component; 8-bit
    quantisation tables; DC and AC Huffman tables 0 and 1; several tables in one ``DQT`` / ``DHT``; any ``APPn`` / ``COM``
    and fill 0xFF bytes; ``DRI`` 0.  Everything else -- progressive, extended, lossless and arithmetic frames, other samplings, a
    restart interval, ``APP14`` Adobe, 16-bit tables, four components, H = 0 (``DNL``), more than one scan -- gives its reason.

    The description: dict(H, W, ncomp, mode, qt uint8 [3, 64] natural order per component, dc / ac {id: (bits, vals)},
    comp_dc / comp_ac [3], scan_offset, tables = the ``DECODE_TABLE_BYTES`` block ``kgdet_jpeg_decode`` reads).

    ``camera=True`` (the files cameras and phones write; ``kgdet_jpeg_decode_camera``) additionally takes three components
    sampled 2x1 / 1x1 / 1x1 (4:2:2, ``MODE_422``: an MCU is 16 wide and 8 high, its blocks Y left, Y right, Cb, Cr) and a ``DRI``
    with a non-zero interval; the description then carries ``restart_interval`` (MCUs, 0: none).  Everything else keeps its
    reason, and without the switch the result is what it was."""
    data = bytes(data)
    if data[:2] != b'\xff\xd8':
        return 'no SOI marker'
    at, size = 2, len(data)
    qt, dc, ac = {}, {}, {}
    sof, jfif, restart = None, False, 0
    while True:
        if at + 4 > size:
            return 'the file ends inside its header'
        if data[at] != 0xFF:
            return 'no marker at byte %d' % at
        while data[at + 1] == 0xFF:                     # fill bytes
            at += 1
            if at + 4 > size:
                return 'the file ends inside its header'
        marker = data[at + 1]
        if marker == 0xD9:
            return 'EOI before any scan'
        if marker == 0x01 or 0xD0 <= marker <= 0xD7:
            return 'marker %02X in the header' % marker
        n = data[at + 2] << 8 | data[at + 3]
        if n < 2 or at + 2 + n > size:
            return 'segment %02X runs past the file' % marker
        body = data[at + 4:at + 2 + n]
        if marker == 0xE0:
            jfif = jfif or body[:5] == b'JFIF\x00'
        elif marker == 0xEE and body[:5] == b'Adobe':
            return 'APP14 Adobe segment (its colour transform is not read)'
        elif 0xE0 <= marker <= 0xEF or marker == 0xFE:
            pass
        elif marker == 0xDB:
            k = 0
            while k < len(body):
                pq, tq = body[k] >> 4, body[k] & 15
                if pq != 0:
                    return '16-bit quantisation table'
                if tq > 3 or k + 65 > len(body):
                    return 'malformed DQT segment'
                table = np.zeros(64, dtype=np.uint8)
                table[ZIGZAG] = list(body[k + 1:k + 65])
                qt[tq] = table
                k += 65
        elif marker == 0xC4:
            k = 0
            while k < len(body):
                tc, th = body[k] >> 4, body[k] & 15
                if k + 17 > len(body):
                    return 'malformed DHT segment'
                bits = list(body[k + 1:k + 17])
                count = sum(bits)
                if tc > 1 or k + 17 + count > len(body) or count > (256 if tc else 16) or not _kraft_ok(bits):
                    return 'malformed DHT segment'
                if th > 1:
                    return 'Huffman table %d (tables 0 and 1 are read)' % th
                (ac if tc else dc)[th] = (bits, list(body[k + 17:k + 17 + count]))
                k += 17 + count
        elif marker == 0xC0:
            if sof is not None:
                return 'two frame headers'
            if n < 8 or n != 8 + 3 * body[5]:
                return 'malformed SOF0 segment'
            comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(body[5])]
            sof = (body[0], body[1] << 8 | body[2], body[3] << 8 | body[4], comps)
        elif marker in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF):
            kind = {0xC1: 'extended sequential', 0xC2: 'progressive', 0xC3: 'lossless'}.get(marker, 'arithmetic-coded' if marker >= 0xC9
                                                                                             else 'differential')
            return '%s frame (SOF%d)' % (kind, marker - 0xC0) if marker != 0xCC else 'arithmetic coding (DAC)'
        elif marker == 0xDD:
            if n != 4:
                return 'malformed DRI segment'
            restart = body[0] << 8 | body[1]
            if restart and not camera:
                return 'restart interval %d (DRI)' % restart
        elif marker == 0xDC:
            return 'DNL segment'
        elif marker == 0xDA:
            break
        else:
            return 'unexpected marker %02X' % marker
        at += 2 + n
    if sof is None:
        return 'SOS before the frame header'
    precision, H, W, comps = sof
    if precision != 8:
        return '%d-bit samples' % precision
    if H == 0:
        return 'H = 0 (the height comes in a DNL segment)'
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        return 'image of %d x %d (sides 1 .. %d)' % (H, W, MAX_SIDE)
    if len(comps) == 4:
        return 'four components'
    if len(comps) not in (1, 3):
        return '%d components' % len(comps)
    sampling = [c[1:3] for c in comps]
    if len(comps) == 1:
        mode = MODE_GREY
    elif sampling == [(2, 2), (1, 1), (1, 1)]:
        mode = MODE_420
    elif sampling == [(1, 1), (1, 1), (1, 1)]:
        mode = MODE_444
    elif camera and sampling == [(2, 1), (1, 1), (1, 1)]:
        mode = MODE_422
    else:
        return 'sampling %s (2x2 / 1x1 / 1x1 and 1x1 / 1x1 / 1x1 are read)' % ' / '.join('%dx%d' % s for s in sampling)
    if len(comps) == 3 and not (jfif or [c[0] for c in comps] == [1, 2, 3]):
        return 'three components that are not marked as YCbCr (no JFIF APP0, ids %s)' % ', '.join(str(c[0]) for c in comps)
    if n < 6 or body[0] < 1 or n != 6 + 2 * body[0]:
        return 'malformed SOS segment'
    if body[0] != len(comps):
        return 'more than one scan (a scan of %d of %d components)' % (body[0], len(comps))
    comp_dc, comp_ac = [0, 0, 0], [0, 0, 0]
    for i, c in enumerate(comps):
        cid, td, ta = body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15
        if cid != c[0]:
            return 'the scan names component %d where the frame has %d' % (cid, c[0])
        if td not in dc or ta not in ac:
            return 'the scan names a Huffman table the file does not define'
        if c[3] not in qt:
            return 'the frame names a quantisation table the file does not define'
        comp_dc[i], comp_ac[i] = td, ta
    if tuple(body[1 + 2 * body[0]:]) != (0, 63, 0):
        return 'spectral selection or successive approximation in a baseline scan'
    Q = np.stack([qt[comps[min(i, len(comps) - 1)][3]] for i in range(3)])
    blob = bytearray(DECODE_TABLE_BYTES)
    blob[0:192] = Q.tobytes()
    for t in range(2):
        for tables, bits_at, vals_at, room in ((dc, 192, 224, 16), (ac, 256, 288, 256)):
            if t in tables:
                bits, vals = tables[t]
                blob[bits_at + 16 * t:bits_at + 16 * t + 16] = bytes(bits)
                blob[vals_at + room * t:vals_at + room * t + len(vals)] = bytes(vals)
    blob[800:803], blob[803:806] = bytes(comp_dc), bytes(comp_ac)
    frame = dict(H=H, W=W, ncomp=len(comps), mode=mode, qt=Q, dc=dc, ac=ac, comp_dc=comp_dc, comp_ac=comp_ac,
                 scan_offset=at + 2 + n, tables=bytes(blob))
    if camera:
        frame['restart_interval'] = restart
    return frame


def frame_blocks(frame):
    """(MCUs per row, MCU rows, blocks per MCU) of a frame; a one-component scan is not padded to an MCU: its MCU is a block"""
    wide = 16 if frame['mode'] in (MODE_420, MODE_422) else 8
    high = 16 if frame['mode'] == MODE_420 else 8
    return (frame['W'] + wide - 1) // wide, (frame['H'] + high - 1) // high, BLOCKS_PER_MCU[frame['mode']]


def unstuff(data, scan_offset):
    """the scan's bytes with the 0xFF 0x00 stuffing removed: it ends at the first 0xFF that a byte other than 0x00 follows, which
    has to be ``EOI``; bytes behind it are ignored"""
    k = data.find(b'\xff', scan_offset)
    while k >= 0 and k + 1 < len(data) and data[k + 1] == 0:
        k = data.find(b'\xff', k + 2)
    if k < 0 or k + 1 >= len(data):
        raise ValueError('no marker ends the scan')
    if data[k + 1] != 0xD9:
        raise ValueError('marker %02X ends the scan, not EOI' % data[k + 1])
    return data[scan_offset:k].replace(b'\xff\x00', b'\xff')


def unstuff_intervals(data, scan_offset):
    """``unstuff`` for a scan with restart intervals: the scan's data is cut at every 0xFF 0xD0+m and each piece is un-stuffed
    on its own -> (the pieces, the marker numbers m in file order).  The scan ends at the first 0xFF that neither 0x00 nor a
    restart marker follows (a second 0xFF included: no fill bytes here), which has to be ``EOI``."""
    pieces, markers, at = [], [], scan_offset
    k = data.find(b'\xff', scan_offset)
    while k >= 0 and k + 1 < len(data) and (data[k + 1] == 0 or 0xD0 <= data[k + 1] <= 0xD7):
        if data[k + 1]:
            pieces.append(data[at:k].replace(b'\xff\x00', b'\xff'))
            markers.append(data[k + 1] - 0xD0)
            at = k + 2
        k = data.find(b'\xff', k + 2)
    if k < 0 or k + 1 >= len(data):
        raise ValueError('no marker ends the scan')
    if data[k + 1] != 0xD9:
        raise ValueError('marker %02X ends the scan, not EOI' % data[k + 1])
    pieces.append(data[at:k].replace(b'\xff\x00', b'\xff'))
    return pieces, markers


def _lookup(bits, vals):
    """(symbol, length) by the next 16 bits: two lists of 65536, length 0 where no code matches"""
    sym, length_of = np.zeros(65536, dtype=np.int64), np.zeros(65536, dtype=np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            lo = code << (16 - length)
            sym[lo:lo + (1 << (16 - length))] = vals[k]
            length_of[lo:lo + (1 << (16 - length))] = length
            code, k = code + 1, k + 1
        code <<= 1
    return sym.tolist(), length_of.tolist()


class EntropyContext(object):
    """the un-stuffed stream of a file with what ``decode_span`` needs: ``window[p]`` = the 32 bits from bit p (1-bits behind the
    end), the look-ups of each block slot of the MCU, ``total_bits``"""

    def __init__(self, frame, stream, tables=None):
        """``tables``: a context of the same frame whose look-ups are shared (the intervals of one file)"""
        self.frame, self.stream, self.total_bits = frame, stream, 8 * len(stream)
        bit = np.unpackbits(np.frombuffer(stream + b'\xff' * 5, dtype=np.uint8)).astype(np.int64)
        window = np.zeros(self.total_bits + 1, dtype=np.int64)
        for j in range(32):
            window += bit[j:j + self.total_bits + 1] << (31 - j)
        self.window = window.tolist()
        self.bpm = BLOCKS_PER_MCU[frame['mode']]
        comp = SLOT_COMPONENT[frame['mode']]
        if tables is not None:
            self.slot_comp, self.slot_tables = tables.slot_comp, tables.slot_tables
            return
        luts = {}
        for kind, tables in (('dc', frame['dc']), ('ac', frame['ac'])):
            for t, (bits, vals) in tables.items():
                luts[kind, t] = _lookup(bits, vals)
        self.slot_comp = comp
        self.slot_tables = [(luts['dc', frame['comp_dc'][c]], luts['ac', frame['comp_ac'][c]]) for c in comp]


def decode_span(ctx, state, limit, sink=None, trace=None):
    """Decode the symbols that START before bit ``limit`` from ``state`` = (bit position, block slot inside the MCU, zigzag
    index; index 0: the next symbol is a DC code) -> (the exit state, blocks completed).  This is the step the Huffman kernel
    takes per lane, for a true state and for a speculative one alike:
    - a symbol (code and magnitude bits) that would run past the stream's last bit is not taken, and neither is an unmatched
      code within the last 15 bits (read with 1-bits behind the end, no code fits what is left): the span stops in front of it;
    - an unmatched code, a DC category above 11, an AC category above 10, a (run, 0) symbol other than EOB and ZRL, and a zigzag
      index past 63 (a ZRL that reaches the block's end included) give ``INVALID``; ``INVALID`` stays ``INVALID``.
    ``sink(block, zigzag index, value)`` receives the coefficients (a DC value is the difference), ``block`` counted from the
    span's start; ``trace`` (a list) receives (position, code bits, magnitude bits, symbol, zigzag index, block completed)."""
    if state == INVALID:
        return INVALID, 0
    p, b, z = state
    done, total, window, bpm = 0, ctx.total_bits, ctx.window, ctx.bpm
    while p < limit and p < total:
        w = window[p]
        (dsym, dlen), (asym, alen) = ctx.slot_tables[b]
        ends = False
        if z == 0:
            length = dlen[w >> 16]
            if length == 0:
                if total - p < 16:
                    break
                return INVALID, done
            s = run = dsym[w >> 16]
            if s > 11:
                return INVALID, done
            place = 0
        else:
            length = alen[w >> 16]
            if length == 0:
                if total - p < 16:
                    break
                return INVALID, done
            rs = asym[w >> 16]
            run, s = rs >> 4, rs & 15
            if s == 0:
                if run == 15:
                    if z + 16 > 63:
                        return INVALID, done
                elif run != 0:
                    return INVALID, done
            else:
                if z + run > 63 or s > 10:
                    return INVALID, done
            place = z + run
        if p + length + s > total:
            break
        if z == 0 or s:
            if s:
                v = (w >> (32 - length - s)) & ((1 << s) - 1)
                if not v >> (s - 1):
                    v -= (1 << s) - 1
            else:
                v = 0
            if sink is not None and (s or z == 0):
                sink(done, place, v)
            nz = place + 1
            ends = nz == 64
        elif run == 15:
            nz = z + 16
        else:
            nz, ends = 0, True
        if trace is not None:
            trace.append((p, length, s, -1 if z == 0 else (run << 4 | s), z, ends))
        p += length + s
        if ends:
            z = 0
            b = b + 1 if b + 1 < bpm else 0
            done += 1
        else:
            z = nz
    return (p, b, z), done


def _idct_1d(x, shift):
    """libjpeg's jidctint.c (islow) butterfly along the last axis of int64 [..., 8], then (v + 2^(shift - 1)) >> shift"""
    F = IDCT_CONST
    i0, i1, i2, i3, i4, i5, i6, i7 = [x[..., n] for n in range(8)]
    z1 = (i2 + i6) * F['c0_541']
    t2, t3 = z1 - i6 * F['c1_847'], z1 + i2 * F['c0_765']
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = i7, i5, i3, i1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * F['c1_175']
    o0, o1, o2, o3 = o0 * F['c0_298'], o1 * F['c2_053'], o2 * F['c3_072'], o3 * F['c1_501']
    z1, z2 = -z1 * F['c0_899'], -z2 * F['c2_562']
    z3, z4 = -z3 * F['c1_961'] + z5, -z4 * F['c0_390'] + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    out = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    return np.stack([(v + (1 << (shift - 1))) >> shift for v in out], axis=-1)


def idct_blocks(levels, q):
    """int64 [a, b, 8, 8] levels and a table [64] (natural order) -> the samples int64 [8 a, 8 b] in 0 .. 255"""
    a, b = levels.shape[:2]
    f = levels.astype(np.int64) * q.reshape(8, 8).astype(np.int64)
    ws = _idct_1d(f.transpose(0, 1, 3, 2), 11).transpose(0, 1, 3, 2)        # pass 1: down the columns
    out = _idct_1d(ws, 18) + 128                                            # pass 2: along the rows
    return np.clip(out, 0, 255).transpose(0, 2, 1, 3).reshape(8 * a, 8 * b)


def fancy_upsample_h2v1(c, cw):
    """libjpeg's triangle ("fancy") h2v1 upsampling of the real extent ``cw`` of a chroma plane's rows -> int64 [rows, 2 cw]"""
    c = c[:, :cw].astype(np.int64)
    if cw <= 2:                         # libjpeg replicates a plane of up to two samples a row (at cw = 1 the same values)
        return np.repeat(c, 2, axis=1)
    left, right = np.concatenate([c[:, :1], c[:, :-1]], 1), np.concatenate([c[:, 1:], c[:, -1:]], 1)
    out = np.empty((c.shape[0], 2 * cw), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * c + left + 1) >> 2, (3 * c + right + 2) >> 2
    return out


def fancy_upsample(c, ch, cw):
    """libjpeg's triangle ("fancy") h2v2 upsampling of the real extent [ch, cw] of a chroma plane -> int64 [2 ch, 2 cw]"""
    c = c[:ch, :cw].astype(np.int64)
    up, dn = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    rows = np.empty((2 * ch, cw), dtype=np.int64)
    rows[0::2], rows[1::2] = 3 * c + up, 3 * c + dn
    left, right = np.concatenate([rows[:, :1], rows[:, :-1]], 1), np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
    out = np.empty((2 * ch, 2 * cw), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * rows + left + 8) >> 4, (3 * rows + right + 7) >> 4
    return out


def decode_parts(data, trace=None, camera=False):
    """the restatement with its intermediate results: dict(frame, stream, coefficients int64 [blocks, 64] natural order in
    scan order with the DC values summed, planes, image); ``camera``: ``parse_header``'s switch (``stream`` is then the
    intervals' un-stuffed bytes one after the other and ``intervals`` their lengths)"""
    data = bytes(data)
    frame = parse_header(data, camera)
    if isinstance(frame, str):
        raise ValueError('decode_restatement does not read this file: %s' % frame)
    mw, mh, bpm = frame_blocks(frame)
    nblocks = mw * mh * bpm
    zz = np.zeros((nblocks + 1, 64), dtype=np.int64)
    interval = frame.get('restart_interval', 0)
    if interval:
        pieces, markers = unstuff_intervals(data, frame['scan_offset'])
        count = -(-mw * mh // interval)
        if len(pieces) != count:
            raise ValueError('%d restart markers in a scan of %d intervals' % (len(markers), count))
        if markers != [m % 8 for m in range(count - 1)]:
            raise ValueError('the restart markers do not count 0 .. 7 in turn: %s' % markers)
    else:
        pieces = [unstuff(data, frame['scan_offset'])]
    stream = b''.join(pieces)
    ctx, first = None, 0
    for k, piece in enumerate(pieces):
        ctx = EntropyContext(frame, piece, ctx)
        share = min(nblocks - first, interval * bpm) if interval else nblocks

        def sink(block, place, value):
            zz[first + block if block < share else nblocks, place] = value
        state, done = decode_span(ctx, (0, 0, 0), ctx.total_bits, sink, trace)
        if state == INVALID:
            raise ValueError('the scan holds an invalid code')
        if done != share or state[2] != 0 or not 0 <= ctx.total_bits - state[0] < 8:
            if interval:
                raise ValueError('interval %d holds %d blocks and ends %d bits before its data does; its share is %d blocks'
                                 % (k, done, ctx.total_bits - state[0], share))
            raise ValueError('the scan holds %d blocks and ends %d bits before its data does; the frame has %d blocks'
                             % (done, ctx.total_bits - state[0], nblocks))
        first += share
    ctx = EntropyContext(frame, stream, ctx) if interval else ctx
    zz = zz[:nblocks].reshape(mw * mh, bpm, 64)
    comp = np.array(SLOT_COMPONENT[frame['mode']])
    for at in range(0, mw * mh, interval or mw * mh):                           # the running sums start at 0 in every interval
        for c in range(frame['ncomp']):
            dc = zz[at:at + (interval or mw * mh), comp == c, 0]
            zz[at:at + (interval or mw * mh), comp == c, 0] = np.cumsum(dc.reshape(-1)).reshape(dc.shape)
    zz = np.clip(zz, -32768, 32767)
    coef = np.zeros_like(zz)
    coef[..., ZIGZAG] = zz
    grid = coef.reshape(mh, mw, bpm, 8, 8)
    H, W, Q = frame['H'], frame['W'], frame['qt']
    if frame['mode'] == MODE_420:
        luma = grid[:, :, :4].reshape(mh, mw, 2, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(2 * mh, 2 * mw, 8, 8)
        ch, cw = (H + 1) // 2, (W + 1) // 2
        planes = [idct_blocks(luma, Q[0])[:H, :W]] + [fancy_upsample(idct_blocks(grid[:, :, 3 + c], Q[c]), ch, cw)[:H, :W]
                                                     for c in (1, 2)]
    elif frame['mode'] == MODE_422:
        luma = grid[:, :, :2].reshape(mh, 2 * mw, 8, 8)
        planes = [idct_blocks(luma, Q[0])[:H, :W]] + [fancy_upsample_h2v1(idct_blocks(grid[:, :, 1 + c], Q[c]), (W + 1) // 2)[:H, :W]
                                                     for c in (1, 2)]
    else:
        planes = [idct_blocks(grid[:, :, c], Q[c])[:H, :W] for c in range(bpm)]
    if frame['mode'] == MODE_GREY:
        rgb = np.stack([planes[0]] * 3, -1)
    else:
        Y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
        rgb = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                        Y + ((116130 * cb + 32768) >> 16)], -1)
    image = np.clip(rgb, 0, 255).astype(np.uint8)
    out = dict(frame=frame, stream=stream, context=ctx, coefficients=coef.reshape(nblocks, 64), planes=planes, image=image)
    if camera:
        out['intervals'] = [len(piece) for piece in pieces]
    return out


def decode_restatement(data, camera=False):
    """The picture of a JPEG file ``parse_header`` takes -> uint8 [H, W, 3] RGB: the definition ``kgdet_jpeg_decode`` is held to
    bit for bit, itself held to PIL's decoder (libjpeg-turbo), which is what ``DeepFashion2Dataset.load_image`` returns.

    1. Entropy layer: ``unstuff``, then ``decode_span`` from (0, 0, 0) over the whole stream.  The scan has to hold exactly the
       frame's blocks and end within the last byte of its data; the DC values are the running sums of the differences per
       component.  Levels are clamped to -32768 .. 32767 (a file made from pixels stays within +-2048).
    2. Dequantisation, level * q in natural order.
    3. libjpeg's ``islow`` inverse DCT (CONST_BITS 13, PASS1_BITS 2, the constants ``IDCT_CONST``): pass 1 down the columns with
       (x + 2^10) >> 11, pass 2 along the rows with (x + 2^17) >> 18, + 128, clamped to 0 .. 255.
    4. Chroma of 2x2-sampled files: libjpeg's "fancy" triangle upsampling over the real extent ceil(H / 2) x ceil(W / 2):
       v = 3 c[r] + c[r -/+ 1] for the upper / lower output row, then (3 v[x] + v[x - 1] + 8) >> 4 for an even and
       (3 v[x] + v[x + 1] + 7) >> 4 for an odd output column, the neighbour replicated at every edge.
    5. Colour, cb and cr the samples minus 128, arithmetic shifts, clamped: R = Y + ((91881 cr + 32768) >> 16),
       G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16); one component gives R = G = B = Y.

    Pinned domain: equality with PIL holds for files an encoder made from pixels (tests/test_jpeg_decode_refs.py).  A patched
    file whose dequantised coefficients overflow 16-bit intermediates is outside it: libjpeg-turbo's SIMD inverse DCT wraps
    there, where this definition (64-bit integers) and the kernels clamp and agree with each other.  Raises ``ValueError``
    for a file ``parse_header`` refuses and for a scan that is malformed; PIL is more lenient with both.

    ``camera=True`` (``parse_header``'s switch; ``kgdet_jpeg_decode_camera``'s definition):
    - Restart intervals.  The scan's data is cut at every 0xFF 0xD0+m (``unstuff_intervals``); the markers must count m = 0, 1,
      .. 7, 0, .. and there are exactly ceil(MCUs / interval) - 1 of them before ``EOI``.  Each piece is un-stuffed on its own
      and decoded by ``decode_span`` from (0, 0, 0); it has to hold exactly its share of blocks (interval * blocks per MCU, the
      last piece the remainder) and end within the last byte of its data; the DC running sums start at 0 in every piece.  The
      look-ups are built once per file.  A violation is a ``ValueError``.
    - 4:2:2 chroma: libjpeg's h2v1 "fancy" upsampling over the real extent ceil(W / 2): out[2x] = (3 c[x] + c[x - 1] + 1) >> 2,
      out[2x + 1] = (3 c[x] + c[x + 1] + 2) >> 2, the neighbour replicated at both edges; rows are not touched.  A plane of
      two samples a row (W = 3, 4) is replicated instead, out[2x] = out[2x + 1] = c[x], as libjpeg does for widths up to 2.
      The luma grid is the MCU's two blocks side by side.  Steps 2, 3 and 5 are unchanged."""
    return decode_parts(data, camera=camera)['image']


def _align(v, a):
    return (v + a - 1) // a * a


def pack_files(files, frames, into=None):
    """Lay the scans (from the first entropy byte to the file's end) and the table blocks of ``files`` out in one buffer, each
    at a multiple of 16 bytes -> (bytes used, [(scan offset, scan bytes, tables offset)]); ``into``: a uint8 numpy array that
    receives them (None: only the layout)"""
    at, places = 0, []
    for data, frame in zip(files, frames):
        scan = len(data) - frame['scan_offset']
        places.append((at, scan, at + _align(scan, 16)))
        if into is not None:
            into[at:at + scan] = np.frombuffer(data, dtype=np.uint8, offset=frame['scan_offset'])
            into[places[-1][2]:places[-1][2] + DECODE_TABLE_BYTES] = np.frombuffer(frame['tables'], dtype=np.uint8)
        at = places[-1][2] + DECODE_TABLE_BYTES
    return at, places


class DeviceJpegDecoder(object):
    """``kgdet_jpeg_decode``.  ``decoder(files)``: ``files`` a list of ``bytes`` that ``parse_header`` takes (``frames``: their
    descriptions, when the caller has parsed them already) -> ``(images, status)``: ``images`` uint8 [H, W, 3] device tensors,
    views of ONE buffer, bit for bit ``decode_restatement``'s; ``status`` the device int32 [n] tensor of the kernels' verdicts
    (0: decoded; else the image's pixels mean nothing).  Nothing is read back here: the caller looks at ``status`` when it
    needs the pictures.  The files travel through one page-locked staging copy and one non-blocking upload, as
    ``DeviceImageTransform._upload``'s images do; everything runs on the device's current stream.  The workspace grows to the
    largest group seen (about 3.5 bytes per pixel of a 4:2:0 picture) and is reused: every call makes its stream wait for the
    event behind the previous call, so the object may be used from any stream (one thread at a time).

    ``camera=True``: ``kgdet_jpeg_decode_camera`` and ``parse_header(camera=True)``'s files -- 4:2:2 and restart intervals as
    well, bit for bit ``decode_restatement(camera=True)``'s; status 4 (``KGDET_JPEG_DECODE_BAD_RESTART``) joins the verdicts."""

    def __init__(self, device=None, camera=False):
        import torch
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.camera = bool(camera)
        self.workspace = None
        self._pinned = None
        self._pinned_free = None
        self._last = None                    # event behind the last call's kernels: the next call's stream waits for it
        self.uploaded = 0                    # bytes of files uploaded so far (tools/time_jpeg_decode.py)

    def __call__(self, files, frames=None):
        import torch
        files = [bytes(f) for f in files]
        frames = [parse_header(f, self.camera) for f in files] if frames is None else list(frames)
        for k, frame in enumerate(frames):
            if isinstance(frame, str):
                raise ValueError('file %d is not one the device decodes: %s' % (k, frame))
        if not files:
            return [], torch.empty(0, dtype=torch.int32, device=self.device)
        total, places = pack_files(files, frames)
        if self._pinned is None or self._pinned.numel() < total:
            self._pinned = torch.empty(max(total, 1 << 20), dtype=torch.uint8, pin_memory=True)
            self._pinned_free = None
        if self._pinned_free is not None:
            self._pinned_free.synchronize()          # (the previous call's upload still reads the buffer)
        pack_files(files, frames, self._pinned.numpy())
        with torch.cuda.device(self.device):
            src = self._pinned[:total].to(self.device, non_blocking=True)
            self._pinned_free = torch.cuda.Event()
            self._pinned_free.record()
        self.uploaded += total
        jobs = [(so, sb, to, f['H'], f['W'], f['mode'], f.get('restart_interval', 0)) for (so, sb, to), f in zip(places, frames)]
        return self.decode(src, jobs)

    def decode(self, src, jobs, out=None, stages=4):
        """the files' bytes already on the device: ``src`` a flat uint8 device tensor, ``jobs`` [(scan offset, scan bytes,
        tables offset, H, W, mode[, restart interval])] with the offsets inside ``src`` (an interval or ``MODE_422`` needs
        ``camera=True``) -> ``(images, status)``; ``out``: a flat uint8 device tensor
        to decode into (the pictures follow each other at multiples of 256 bytes).  ``stages`` < 4 (the timing tool's): only
        the first kernels run, no picture is made and every status is -1.  The workspace is shared by the object's calls: a
        call waits, on the device, for the previous one, whichever stream that ran on."""
        import ctypes
        import torch
        from . import _lib
        lib, p = _lib.lib(), _lib.ptr
        dev = src.device
        jobs = [tuple(j) + (0,) * (7 - len(j)) for j in jobs]
        if not self.camera and any(j[5] == MODE_422 or j[6] for j in jobs):
            raise ValueError('a 4:2:2 file or a restart interval needs DeviceJpegDecoder(camera=True)')
        name = 'kgdet_jpeg_decode_camera' if self.camera else 'kgdet_jpeg_decode'
        workspace_bytes, decode_stages = getattr(lib, name + '_workspace_bytes'), getattr(lib, name + '_stages')
        places, total = [], 0
        for _, _, _, H, W, _, _ in jobs:
            places.append(total)
            total += _align(3 * H * W, 256)
        if out is None:
            out = torch.empty(total, dtype=torch.uint8, device=dev)
        elif not (out.is_cuda and out.device == dev and out.dtype == torch.uint8 and out.dim() == 1 and out.numel() >= total):
            raise ValueError('out must be a flat uint8 tensor of at least %d bytes on %s' % (total, dev))
        status = torch.empty(len(jobs), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            stream = _lib.current_stream()
            if self._last is not None:
                torch.cuda.current_stream().wait_event(self._last)      # (no wait at all on the stream that recorded it)
            for g in range(0, len(jobs), DECODE_MAX_IMAGES):
                group = jobs[g:g + DECODE_MAX_IMAGES]
                table = (_lib.JpegDecodeJob * len(group))(*[
                    _lib.JpegDecodeJob(int(so), int(sb), int(to), places[g + k], int(H), int(W), int(mode), int(interval))
                    for k, (so, sb, to, H, W, mode, interval) in enumerate(group)])
                n = ctypes.c_int32(len(group))
                need = workspace_bytes(table, n)
                if need == 0:
                    _lib.check(_lib.KGDET_E_SHAPE, name + '_workspace_bytes')
                if self.workspace is None or self.workspace.numel() < need or self.workspace.device != dev:
                    self.workspace = None
                    self.workspace = torch.empty(need + need // 4, dtype=torch.uint8, device=dev)
                ws = self.workspace
                _lib.check(decode_stages(p(src), ctypes.c_int64(src.numel()), table, n, p(ws), ctypes.c_size_t(ws.numel()), p(out),
                                         ctypes.c_int64(out.numel()), p(status[g:g + len(group)]), stream, ctypes.c_int32(stages)),
                           name)
            self._last = torch.cuda.Event()
            self._last.record()
        images = [out[at:at + 3 * H * W].view(H, W, 3) for at, (_, _, _, H, W, _, _) in zip(places, jobs)]
        return images, status

    def rounds(self, n):
        """rounds the fixpoint of the last call's first ``n`` images took, the largest over each image's chunks (a read-back)"""
        import torch
        return self.workspace[4 * DECODE_MAX_IMAGES:4 * DECODE_MAX_IMAGES + 4 * n].view(torch.int32).tolist()


def decode_pil(data):
    """the picture of a JPEG file by PIL, as ``DeepFashion2Dataset.load_image`` reads it -> uint8 [H, W, 3] RGB"""
    import io
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert('RGB'))


_decoders = {}


def decode_switch(device_decode):
    """what the loops' ``device_decode`` asks for -> (decode on the device, the ``camera`` switch): False / None, True (the
    baseline files), or 'camera' (4:2:2 files and restart intervals as well)"""
    if device_decode == 'camera':
        return True, True
    if isinstance(device_decode, str):
        raise ValueError("device_decode is False, True or 'camera', got %r" % (device_decode,))
    return bool(device_decode), False           # (any other value by its truth, as before the switch)


def decode_jpeg(data, camera=False):
    """the picture of a JPEG file -> uint8 [H, W, 3] RGB numpy array: by ``DeviceJpegDecoder`` when a GPU and the library are
    there, ``parse_header`` takes the file and the kernels' status is 0; else by PIL.  On the pinned domain (see
    ``decode_restatement``) both give the same bits.  ``camera``: ``parse_header``'s switch."""
    import torch
    data = bytes(data)
    if device_available():
        frame = parse_header(data, camera)
        if not isinstance(frame, str):
            dev = (torch.cuda.current_device(), bool(camera))
            if dev not in _decoders:
                _decoders[dev] = DeviceJpegDecoder(torch.device('cuda', dev[0]), camera)
            images, status = _decoders[dev]([data], [frame])
            if int(status[0]) == 0:
                return images[0].cpu().numpy()
    return decode_pil(data)


class DeviceDecodeRoute(object):
    """What the loader and the test loop do with ``datasets.EncodedImage`` samples: ``route(raws)`` -> the list with every
    ``EncodedImage`` replaced by its picture -- a uint8 [H, W, 3] device tensor from ONE ``kgdet_jpeg_decode`` call per 32 files
    (views of one buffer), or the PIL-decoded host tensor for a file the decoder does not take -- and everything else as it was.
    The list is never handed out before the kernels' status is known: an image with non-zero status is decoded by PIL on the
    spot (which raises for a truncated file exactly as ``load_image`` does) and one warning names the file.

    Upload, decode and the status read-back run on a stream of the route's own, so that the read-back waits for the decode
    alone and never for the work the consumer has queued (a training step); the consumer's current stream is then made to wait
    for the decode's event, and the pictures are marked as used on it (``record_stream``).  ``start_block`` / ``finish_block``: the same in two halves for files
    that already lie in a page-locked block (the loader's ring slot, ``pack_files``' layout at ``files_at``), which goes up in
    one copy together with whatever else the block holds; it returns the device block too.  Between the halves nothing is waited for, so the loader
    starts the next batch's decode while the consumer trains on this one.

    ``camera=True``: the samples' frames come from ``parse_header(camera=True)`` (``load_image_file(idx, camera=True)``) and
    the route decodes with ``kgdet_jpeg_decode_camera``."""

    def __init__(self, device=None, camera=False):
        import torch
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.decoder = DeviceJpegDecoder(self.device, camera)
        self.stream = None
        self._status = None
        self._turn = 0
        self.fallbacks = 0                   # images the kernels refused (decoded by PIL) so far

    def _side(self):
        import torch
        if self.stream is None:
            with torch.cuda.device(self.device):
                self.stream = torch.cuda.Stream()
                self._status = torch.empty((2, DECODE_MAX_IMAGES), dtype=torch.int32).pin_memory()
        return self.stream

    def __call__(self, raws):
        import torch
        raws = list(raws)
        which = [k for k, r in enumerate(raws) if _is_encoded(r) and r.frame is not None]
        out = [torch.from_numpy(np.ascontiguousarray(r.pixels)) if _is_encoded(r) and r.frame is None else r for r in raws]
        for g in range(0, len(which), DECODE_MAX_IMAGES):
            part = which[g:g + DECODE_MAX_IMAGES]
            with torch.cuda.device(self.device):
                consumer = torch.cuda.current_stream()
                with torch.cuda.stream(self._side()):
                    images, status = self.decoder([raws[k].data for k in part], [raws[k].frame for k in part])
                    done = self._read_back(status)
                for k, img in zip(part, self._finish(images, done, [raws[j] for j in part], consumer)):
                    out[k] = img
        return out

    def start_block(self, pinned, files_at, places, raws):
        """``pinned``: the page-locked block; ``places``: ``pack_files``' (scan offset, scan bytes, tables offset) relative to
        ``files_at`` for the ``EncodedImage``s of ``raws`` that have a frame, in order (at most 32).  Issues the block's upload,
        the decode and the status read-back on the route's stream and WAITS FOR NOTHING -> a handle for ``finish_block``, with
        ``uploaded`` (the event behind the block's upload: the block may be written again once it has completed)."""
        import torch
        raws = list(raws)
        which = [k for k, r in enumerate(raws) if _is_encoded(r) and r.frame is not None]
        assert len(which) == len(places) <= DECODE_MAX_IMAGES
        out = [torch.from_numpy(np.ascontiguousarray(r.pixels)) if _is_encoded(r) and r.frame is None else r for r in raws]
        with torch.cuda.device(self.device):
            with torch.cuda.stream(self._side()):
                dev = pinned.to(self.device, non_blocking=True)
                uploaded = torch.cuda.Event()
                uploaded.record()
                images, done, slot = [], None, self._turn
                if which:
                    jobs = [(files_at + so, sb, files_at + to, raws[k].frame['H'], raws[k].frame['W'], raws[k].frame['mode'],
                             raws[k].frame.get('restart_interval', 0)) for k, (so, sb, to) in zip(which, places)]
                    images, status = self.decoder.decode(dev, jobs)
                    self._turn = 1 - slot                # (two handles may be open: each has its own page-locked status)
                    done = self._read_back(status, slot)
        return _Pending(dev, out, which, images, done, [raws[k] for k in which], uploaded, slot)

    def finish_block(self, pending):
        """-> (device block, pictures) of a ``start_block`` handle, on the consumer's current stream: waits for the decode's
        event alone, then PIL for every image the kernels refused"""
        import torch
        with torch.cuda.device(self.device):
            consumer = torch.cuda.current_stream()
            if pending.done is None:
                consumer.wait_event(pending.uploaded)
            else:
                pictures = self._finish(pending.images, pending.done, pending.encoded, consumer, pending.slot)
                for k, img in zip(pending.which, pictures):
                    pending.out[k] = img
            pending.dev.record_stream(consumer)
        return pending.dev, pending.out

    def _read_back(self, status, slot=0):
        """(on the side stream) the status into page-locked memory and the event behind it"""
        import torch
        self._status[slot, :status.numel()].copy_(status, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        return done

    def _finish(self, images, done, encoded, consumer, slot=0):
        import warnings
        import torch
        done.synchronize()                   # the decode's own stream: nothing of the consumer's queue is waited for
        consumer.wait_event(done)
        if images:
            images[0].record_stream(consumer)            # (views of one buffer: one storage)
        out = []
        for img, enc, status in zip(images, encoded, self._status[slot, :len(images)].tolist()):
            if status != 0:
                self.fallbacks += 1
                warnings.warn('%s: the device JPEG decoder refused the scan (status %d); decoded on the host'
                              % (enc.name or 'an image', status))
                img = torch.from_numpy(decode_pil(enc.data))
            out.append(img)
        return out


class _Pending(object):
    """a batch whose upload and decode ``DeviceDecodeRoute.start_block`` has issued"""

    def __init__(self, dev, out, which, images, done, encoded, uploaded, slot):
        self.dev, self.out, self.which, self.images, self.done = dev, out, which, images, done
        self.encoded, self.uploaded, self.slot = encoded, uploaded, slot


def _is_encoded(r):
    from .datasets import EncodedImage
    return isinstance(r, EncodedImage)
