"""Image preprocessing on the device: ``datasets.ImageTransform`` (resize, normalise, flip, pad, CHW) for a whole batch
of raw uint8 images in ONE HIP launch (``csrc/preprocess.hip`` ``kgdet_image_preprocess``).

* ``plan`` -- the geometry ``ImageTransform.__call__`` derives from an image size (new size, ``img_shape``,
  ``pad_shape``, ``scale_factor``), value for value and type for type, without touching pixels.
* ``image_transform_restatement`` -- plain torch / numpy on the CPU: the kernel's arithmetic, bit for bit, and the path for
  host tensors (what ``detector.merge_aug_results_kp`` is for the merge kernel).  ``RestatementImageTransform`` wraps it
  in ``ImageTransform``'s call signature so a dataset can use it as its ``img_transform``.
* ``DeviceImageTransform`` -- the launch: raw images (host ones uploaded through page-locked memory, 3 bytes per pixel
  instead of 12) -> the detector's float32 input on the GPU.
* ``image_transform_restatement_aug`` -- the same under train-time ``extra_aug`` (``augment.AugPlan``): photometric distortion
  on every source pixel, expand / crop as a window in front of the resize; its own contract, below.  The host route of a
  dataset with ``extra_aug`` and the kernel ``kgdet_image_preprocess_aug`` (``csrc/preprocess_aug.hip``) are both held to it.

The arithmetic contract (per axis, ``d`` the index in the un-flipped resized image, ``n`` the source extent, every
operation rounded to float32 on its own, no fused multiply-add)::

    scale = float32(n) / float32(new_n)
    src = max(scale * (d + 0.5) - 0.5, 0);  i0 = min(int(src), n - 1);  i1 = i0 + (i0 < n - 1);  l1 = src - i0;  l0 = 1 - l1
    v = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)
    q = uint8(clamp(round_half_even(v), 0, 255));  out = ((float32(q) - mean[c]) / std[c]) looked up in a [3][256] table

This is ``ImageTransform``'s geometry (``F.interpolate(mode='bilinear', align_corners=False)`` on the float image, rounded to
uint8); torch's CPU kernel orders its sums differently, so the two agree except at rounding ties, where they differ by one
grey level (tests/test_preprocess.py bounds how often).

The ``extra_aug`` contract.  The image is float32 from the first step, as in the reference, so the resize works on floats,
nothing is quantised to a grey level and there is no table: ``out = (v - mean[c]) / std[c]``.  Per source pixel, raw RGB order::

    1. brightness: x + delta                       2. contrast: x * alpha, when the mode is "first"
    3. to HSV  (EPS = 2^-23; max / min taken as ``b > a ? b : a`` / ``b < a ? b : a``):
         v = max(r, g, b); vmin = min(r, g, b); diff = v - vmin; s = diff / (|v| + EPS); d = 60 / (diff + EPS)
         h = (g - b) * d if v == r, else (b - r) * d + 120 if v == g, else (r - g) * d + 240;  if h < 0: h += 360
    4. saturation: s * sat                         5. hue: h + dh; if h > 360: h -= 360; if h < 0: h += 360
    6. to RGB: s == 0 -> r = g = b = v; else h *= float32(6 / 360); while h < 0: h += 6; while h >= 6: h -= 6;
         k = floor(h); f = h - k (k >= 6: k = 0, f = 0); t = [v, v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))]
         (b, g, r) = t[...] by sector k from [(1,3,0), (1,0,2), (3,0,1), (0,2,1), (0,1,3), (2,1,0)]
    7. contrast: x * alpha, when the mode is "last"  8. the channel permutation q

Stages 3 and 6 run whenever photometric distortion is configured (the round trip is not the identity in float32); each of
the others only when it was drawn.  mmcv / cv2 are not available here: the two conversions are THIS project's definition,
restated from OpenCV's float formulas, and parity with cv2 itself is not pinned.  The resize then reads a virtual image V --
the crop patch, else the expand canvas, else the raw image: V[y][x] is the distorted raw pixel (y - oy, x - ox) inside the
raw image and the (undistorted) fill elsewhere -- with the taps of the contract above for n = V's extent, edge-clamped at V's
borders, and ``v = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)`` on the floats.  The fill is the expand's ``mean``
in RGB order; with the normalisation's own mean it normalises to 0 wherever ``lx0 * m + lx1 * m`` is exact (weights 0 / 1, or
dyadic weights on a short mantissa) and to within an ulp of ``m`` over ``std`` elsewhere.
"""
import ctypes
import math

import numpy as np
import torch

from .datasets import rescale_size


def plan(h, w, scale, keep_ratio=True, size_divisor=None):
    """(new_h, new_w, img_shape, pad_shape, scale_factor) of an h x w image: what ``ImageTransform.__call__`` computes and
    returns for it (``scale_factor`` a python float for ``keep_ratio``, else the per-axis float32 array)."""
    if keep_ratio:
        new_h, new_w, scale_factor = rescale_size(h, w, scale)
    else:
        new_w, new_h = scale
        scale_factor = np.array([new_w / w, new_h / h, new_w / w, new_h / h], dtype=np.float32)
    img_shape = (int(new_h), int(new_w), 3)
    if size_divisor is not None:
        pad_shape = (int(math.ceil(img_shape[0] / size_divisor)) * size_divisor,
                     int(math.ceil(img_shape[1] / size_divisor)) * size_divisor, 3)
    else:
        pad_shape = img_shape
    return new_h, new_w, img_shape, pad_shape, scale_factor


def axis_scale(n, new_n):
    """the resize factor of one axis as the kernel takes it: float32(n) / float32(new_n), rounded once"""
    return np.float32(n) / np.float32(new_n)


def norm_table(mean, std):
    """[3, 256] float32: numpy's own ``(float32(q) - mean[c]) / std[c]`` -- the normalisation of ``ImageTransform`` for
    every grey level, so a lookup equals its bits by construction"""
    mean = np.asarray(mean, dtype=np.float32).reshape(3, 1)
    std = np.asarray(std, dtype=np.float32).reshape(3, 1)
    return (np.arange(256, dtype=np.float32)[None, :] - mean) / std


def _taps(n, new_n):
    d = torch.arange(new_n, dtype=torch.float32)
    src = ((d + 0.5) * float(axis_scale(n, new_n)) - 0.5).clamp_(min=0)
    i0 = src.to(torch.int64).clamp_(max=n - 1)
    i1 = i0 + (i0 < n - 1).to(torch.int64)
    l1 = src - i0.to(torch.float32)
    return i0, i1, 1 - l1, l1


def resize_restatement_u8(img_u8, new_h, new_w):
    """uint8 H x W x 3 (numpy or CPU tensor) -> uint8 tensor new_h x new_w x 3 by the contract's bilinear arithmetic"""
    t = torch.as_tensor(np.ascontiguousarray(img_u8) if isinstance(img_u8, np.ndarray) else img_u8)
    assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3 and not t.is_cuda
    y0, y1, ly0, ly1 = _taps(t.shape[0], new_h)
    x0, x1, lx0, lx1 = _taps(t.shape[1], new_w)
    f = t.to(torch.float32)
    top, bot = f[y0], f[y1]
    lx0, lx1 = lx0[None, :, None], lx1[None, :, None]
    v = ly0[:, None, None] * (lx0 * top[:, x0] + lx1 * top[:, x1]) + ly1[:, None, None] * (lx0 * bot[:, x0] + lx1 * bot[:, x1])
    return v.round_().clamp_(0, 255).to(torch.uint8)


def image_transform_restatement(img_u8, scale, flip=False, keep_ratio=True, mean=(0, 0, 0), std=(1, 1, 1), to_rgb=True,
                                size_divisor=None, out_hw=None):
    """``ImageTransform(mean, std, to_rgb, size_divisor)(img_u8, scale, flip, keep_ratio)`` by the contract's arithmetic:
    returns (float32 numpy [3, H, W], img_shape, pad_shape, scale_factor).  ``out_hw``: zero-pad to this (H, W) instead of
    ``pad_shape`` (a batch's common size); ``pad_shape`` itself stays the planned one."""
    h, w = img_u8.shape[:2]
    new_h, new_w, img_shape, pad_shape, scale_factor = plan(h, w, scale, keep_ratio, size_divisor)
    q = resize_restatement_u8(img_u8, img_shape[0], img_shape[1]).to(torch.int64)
    if not to_rgb:
        q = q.flip(-1)
    lut = torch.from_numpy(norm_table(mean, std))
    img = torch.stack([lut[c][q[..., c]] for c in range(3)])          # [3, new_h, new_w]
    if flip:
        img = img.flip(-1)
    H, W = (pad_shape[0], pad_shape[1]) if out_hw is None else out_hw
    assert H >= img_shape[0] and W >= img_shape[1]
    out = np.zeros((3, H, W), dtype=np.float32)
    out[:, :img_shape[0], :img_shape[1]] = img.numpy()
    return out, img_shape, pad_shape, scale_factor


class RestatementImageTransform(object):
    """``image_transform_restatement`` behind ``ImageTransform``'s interface (a drop-in ``dataset.img_transform``)"""

    def __init__(self, mean=(0, 0, 0), std=(1, 1, 1), to_rgb=True, size_divisor=None):
        self.mean = np.array(mean, dtype=np.float32)
        self.std = np.array(std, dtype=np.float32)
        self.to_rgb = to_rgb
        self.size_divisor = size_divisor

    def __call__(self, img, scale, flip=False, keep_ratio=True):
        return image_transform_restatement(img, scale, flip, keep_ratio, self.mean, self.std, self.to_rgb,
                                           self.size_divisor)


_size_plan = plan          # (``image_transform_restatement_aug`` takes the augmentation plan as ``plan``)

HSV_EPS = 2.0 ** -23
HSV_SECTORS = ((1, 3, 0), (1, 0, 2), (3, 0, 1), (0, 2, 1), (0, 1, 3), (2, 1, 0))       # (b, g, r) indices into t, per sector


def _max(a, b):
    return np.where(b > a, b, a)


def _min(a, b):
    return np.where(b < a, b, a)


def rgb_to_hsv_restatement(r, g, b):
    """stage 3 of the ``extra_aug`` contract in the arrays' own dtype (float32: the contract; float64: its exact-ish value)"""
    dt = r.dtype.type
    v = _max(_max(r, g), b)
    vmin = _min(_min(r, g), b)
    diff = v - vmin
    s = diff / (np.abs(v) + dt(HSV_EPS))
    d = dt(60) / (diff + dt(HSV_EPS))
    h = np.where(v == r, (g - b) * d, np.where(v == g, (b - r) * d + dt(120), (r - g) * d + dt(240)))
    h = np.where(h < 0, h + dt(360), h)
    return h, s, v


def hsv_to_rgb_restatement(h, s, v):
    """stage 6 of the ``extra_aug`` contract in the arrays' own dtype"""
    dt = h.dtype.type
    hh = h * dt(6.0 / 360.0)                         # the constant rounded once, to the working precision
    while (hh < 0).any():
        hh = np.where(hh < 0, hh + dt(6), hh)
    while (hh >= 6).any():
        hh = np.where(hh >= 6, hh - dt(6), hh)
    k = np.floor(hh)
    f = hh - k
    f = np.where(k >= 6, dt(0), f)
    k = np.where(k >= 6, 0, k).astype(np.int64)
    t = np.stack([v, v * (dt(1) - s), v * (dt(1) - s * f), v * (dt(1) - s * (dt(1) - f))])
    tab = np.array(HSV_SECTORS)
    pick = lambda col: np.take_along_axis(t, tab[k, col][None], axis=0)[0]
    grey = s == 0
    return np.where(grey, v, pick(2)), np.where(grey, v, pick(1)), np.where(grey, v, pick(0))


def aug_job_numbers(aug):
    """the colour fields of ``kgdet_preproc_aug_job`` for an ``AugPlan``: (flags, delta, alpha, sat, hue, perm), the four
    numbers rounded to float32 once (0 where their stage is off) and ``perm`` the packed RGB permutation"""
    from . import _lib
    flags, q = 0, aug.q
    if aug.colour:
        flags = (_lib.AUG_COLOUR | (_lib.AUG_BRIGHTNESS if aug.delta is not None else 0)
                 | (_lib.AUG_CONTRAST if aug.alpha is not None else 0)
                 | (_lib.AUG_CONTRAST_FIRST if aug.alpha is not None and aug.contrast_first else 0)
                 | (_lib.AUG_SATURATION if aug.sat is not None else 0) | (_lib.AUG_HUE if aug.hue is not None else 0)
                 | (_lib.AUG_PERMUTE if q is not None else 0))
    num = [np.float32(0 if x is None else x) for x in (aug.delta, aug.alpha, aug.sat, aug.hue)]
    perm = (0 | 1 << 2 | 2 << 4) if q is None else (q[0] | q[1] << 2 | q[2] << 4)
    return (flags,) + tuple(num) + (perm,)


def distort_restatement(rgb, aug, conversions=None):
    """stages 1-8 of the ``extra_aug`` contract on a float [..., 3] RGB array, in its dtype (the drawn numbers are rounded
    to float32 first either way).  ``conversions``: (to_hsv(r, g, b) -> (h, s, v), to_rgb(h, s, v) -> (r, g, b)) in place
    of the two restated ones (tests pin the draw and arithmetic order to the reference with the identity there)."""
    from . import _lib
    to_hsv, to_rgb = conversions or (rgb_to_hsv_restatement, hsv_to_rgb_restatement)
    dt = rgb.dtype.type
    flags, delta, alpha, sat, hue, _ = aug_job_numbers(aug)
    if not flags & _lib.AUG_COLOUR:
        return rgb
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    if flags & _lib.AUG_BRIGHTNESS:
        r, g, b = r + dt(delta), g + dt(delta), b + dt(delta)
    first = bool(flags & _lib.AUG_CONTRAST_FIRST)
    if flags & _lib.AUG_CONTRAST and first:
        r, g, b = r * dt(alpha), g * dt(alpha), b * dt(alpha)
    h, s, v = to_hsv(r, g, b)
    if flags & _lib.AUG_SATURATION:
        s = s * dt(sat)
    if flags & _lib.AUG_HUE:
        h = h + dt(hue)
        h = np.where(h > 360, h - dt(360), h)
        h = np.where(h < 0, h + dt(360), h)
    r, g, b = to_rgb(h, s, v)
    if flags & _lib.AUG_CONTRAST and not first:
        r, g, b = r * dt(alpha), g * dt(alpha), b * dt(alpha)
    out = np.stack([r, g, b], axis=-1)
    if flags & _lib.AUG_PERMUTE:
        out = out[..., list(aug.q)]
    return np.ascontiguousarray(out)


def aug_fill(aug, mean, to_rgb):
    """float32 [3]: V outside the raw image, in RGB (raw) order -- the expand's own fill, else the normalisation mean"""
    if aug is not None and aug.fill is not None:
        return np.asarray(aug.fill, dtype=np.float32)
    mean = np.asarray(mean, dtype=np.float32)
    return mean.copy() if to_rgb else mean[::-1].copy()


def image_transform_restatement_aug(img_u8, plan, scale, flip=False, keep_ratio=True, mean=(0, 0, 0), std=(1, 1, 1),
                                    to_rgb=True, size_divisor=None, out_hw=None, conversions=None):
    """``image_transform_restatement`` under ``extra_aug``: ``plan`` an ``augment.AugPlan`` (``None``: the identity window, no
    colour stage) -- the module docstring's ``extra_aug`` contract in numpy float32, every operation rounded on its own.
    Returns (float32 numpy [3, H, W], img_shape, pad_shape, scale_factor), the shapes those of the VIRTUAL image."""
    raw = img_u8.numpy() if isinstance(img_u8, torch.Tensor) else np.asarray(img_u8)
    assert raw.dtype == np.uint8 and raw.ndim == 3 and raw.shape[2] == 3
    h, w = raw.shape[:2]
    mean32, std32 = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    f = raw.astype(np.float32)
    if plan is None:
        (vh, vw), (oy, ox) = (h, w), (0, 0)
    else:
        assert (plan.h, plan.w) == (h, w), 'the plan was drawn for a %d x %d image' % (plan.h, plan.w)
        f = distort_restatement(f, plan, conversions)
        (vh, vw), (oy, ox) = plan.virtual_hw, plan.origin
    fill = aug_fill(plan, mean32, to_rgb)
    new_h, new_w, img_shape, pad_shape, scale_factor = _size_plan(vh, vw, scale, keep_ratio, size_divisor)
    y0, y1, ly0, ly1 = [t.numpy() for t in _taps(vh, img_shape[0])]
    x0, x1, lx0, lx1 = [t.numpy() for t in _taps(vw, img_shape[1])]

    def tap(iy, ix):
        ry, rx = iy - oy, ix - ox
        inside = ((ry >= 0) & (ry < h))[:, None] & ((rx >= 0) & (rx < w))[None, :]
        px = f[np.clip(ry, 0, h - 1)][:, np.clip(rx, 0, w - 1)]
        return np.where(inside[..., None], px, fill)

    lx0, lx1, ly0, ly1 = lx0[None, :, None], lx1[None, :, None], ly0[:, None, None], ly1[:, None, None]
    v = ly0 * (lx0 * tap(y0, x0) + lx1 * tap(y0, x1)) + ly1 * (lx0 * tap(y1, x0) + lx1 * tap(y1, x1))
    if not to_rgb:
        v = v[..., ::-1]
    img = ((v - mean32) / std32).transpose(2, 0, 1)
    assert img.dtype == np.float32
    if flip:
        img = img[:, :, ::-1]
    H, W = (pad_shape[0], pad_shape[1]) if out_hw is None else out_hw
    assert H >= img_shape[0] and W >= img_shape[1]
    out = np.zeros((3, H, W), dtype=np.float32)
    out[:, :img_shape[0], :img_shape[1]] = img
    return out, img_shape, pad_shape, scale_factor


class DeviceImageTransform(object):
    """``ImageTransform`` for a batch on the GPU.

    ``transform(raws, scales, flips, keep_ratio=True, out=None, common_size=None)`` -> ``(img, metas)``: ``raws`` uint8
    H x W x 3 tensors (numpy arrays are taken too), one per job; ``scales`` / ``flips`` one per job.  ``img`` is the cuda
    float32 [B, 3, H, W] batch, ``metas`` the per-image ``(img_shape, pad_shape, scale_factor)`` of ``ImageTransform``.
    Every planned ``pad_shape`` must be the same (H, W) unless ``common_size`` is given: ``True`` pads every image to the
    batch's largest ``pad_shape`` (what ``datasets.collate`` does), an ``(H, W)`` pair to that size.  ``out``: write into
    this cuda float32 [B, 3, H, W] tensor (last dimension contiguous), e.g. ``graphed_test_batch``'s ``run.static_img``;
    every element of it is written.

    Host images are packed into one page-locked buffer and uploaded with one ``non_blocking`` copy; images already on the
    device are read where they are (any row pitch).  The SAME tensor object given for several jobs (multi-scale / flip
    TTA) is uploaded once and read by all of them.  One kernel launch per call (per ``PREPROC_MAX_JOBS`` jobs).  Work is
    issued on the current stream of ``device``.  ``separate(...)`` is the same launch with one [1, 3, H_a, W_a] tensor per
    job, each at its own ``pad_shape`` (the input list of ``aug_test``).  A missing library is an error: there is no
    fallback (host tensors that should stay on the host go through ``image_transform_restatement``).

    ``aug_plans`` (on ``__call__`` and ``separate``): one ``augment.AugPlan`` or ``None`` per job -- train-time ``extra_aug``.
    All ``None`` (or no list) is the launch above.  With any plan in the list EVERY job of the call goes through
    ``kgdet_image_preprocess_aug`` (``PREPROC_AUG_MAX_JOBS`` jobs per launch), a ``None`` entry as the identity window with
    no colour stage; the planned shapes are then those of each job's virtual image (``image_transform_restatement_aug``)."""

    def __init__(self, mean=(0, 0, 0), std=(1, 1, 1), to_rgb=True, size_divisor=None, device=None):
        self.mean = np.array(mean, dtype=np.float32)
        self.std = np.array(std, dtype=np.float32)
        self.to_rgb = to_rgb
        self.size_divisor = size_divisor
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self._lut = {}
        self._pinned = None
        self._pinned_free = None          # event: the last upload out of the page-locked buffer has finished

    def lut(self):
        key = (self.mean.tobytes(), self.std.tobytes(), self.device)
        if key not in self._lut:
            self._lut[key] = torch.from_numpy(norm_table(self.mean, self.std)).to(self.device)
        return self._lut[key]

    def plan(self, raw, scale, keep_ratio=True):
        return plan(raw.shape[0], raw.shape[1], scale, keep_ratio, self.size_divisor)

    def _upload(self, raws):
        """device tensors for ``raws`` (one per distinct object), host ones through one page-locked staging copy"""
        srcs, host = {}, []
        for r in raws:
            if id(r) in srcs:
                continue
            t = torch.from_numpy(np.ascontiguousarray(r)) if isinstance(r, np.ndarray) else r
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
                raise ValueError('raw images are uint8 H x W x 3, got %s %s' % (t.dtype, tuple(t.shape)))
            if t.is_cuda:
                if t.device != self.device:
                    raise ValueError('raw image on %s, transform on %s' % (t.device, self.device))
                if t.stride(2) != 1 or t.stride(1) != 3:
                    t = t.contiguous()
                srcs[id(r)] = t
            else:
                srcs[id(r)] = None
                host.append((id(r), t))
        if host:
            offs, total = [], 0
            for _, t in host:
                offs.append(total)
                total += (t.numel() + 255) // 256 * 256
            if self._pinned is None or self._pinned.numel() < total:
                self._pinned = torch.empty(max(total, 1 << 20), dtype=torch.uint8, pin_memory=True)
                self._pinned_free = None
            if self._pinned_free is not None:
                self._pinned_free.synchronize()      # (the previous call's upload still reads the buffer)
            for (_, t), o in zip(host, offs):
                self._pinned[o:o + t.numel()].view(t.shape).copy_(t)
            with torch.cuda.device(self.device):
                dev = self._pinned[:total].to(self.device, non_blocking=True)
                self._pinned_free = torch.cuda.Event()
                self._pinned_free.record()
            for (key, t), o in zip(host, offs):
                srcs[key] = dev[o:o + t.numel()].view(t.shape)
        return [srcs[id(r)] for r in raws]

    @staticmethod
    def job_tables(srcs, plans, flips, dsts):
        """the launches' ``kgdet_preproc_job`` arrays (at most PREPROC_MAX_JOBS jobs each); ``srcs`` device uint8 H x W x 3
        (any row pitch), ``dsts`` [3, out_h, out_w] float32 views with a contiguous last dimension"""
        from . import _lib
        tables = []
        for lo in range(0, len(srcs), _lib.PREPROC_MAX_JOBS):
            hi = min(len(srcs), lo + _lib.PREPROC_MAX_JOBS)
            jobs = (_lib.PreprocJob * (hi - lo))()
            for k in range(lo, hi):
                s, d, (new_h, new_w, _, _, _) = srcs[k], dsts[k], plans[k]
                assert s.is_cuda and s.dtype == torch.uint8 and s.stride(2) == 1 and s.stride(1) == 3
                assert d.is_cuda and d.dtype == torch.float32 and d.dim() == 3 and d.shape[0] == 3 and d.stride(2) == 1
                jobs[k - lo] = _lib.PreprocJob(
                    s.data_ptr(), s.shape[0], s.shape[1], s.stride(0), d.data_ptr(), d.stride(0), d.stride(1),
                    int(new_h), int(new_w), d.shape[1], d.shape[2], float(axis_scale(s.shape[0], new_h)),
                    float(axis_scale(s.shape[1], new_w)), 1 if flips[k] else 0)
            tables.append(jobs)
        return tables

    def launch_tables(self, tables):
        """one ``kgdet_image_preprocess`` launch per table on the device's current stream"""
        from . import _lib
        lut, L = self.lut(), _lib.lib()
        with torch.cuda.device(self.device):
            stream = _lib.current_stream()
            for jobs in tables:
                _lib.check(L.kgdet_image_preprocess(jobs, ctypes.c_int32(len(jobs)), _lib.ptr(lut),
                                                    ctypes.c_int32(0 if self.to_rgb else 1), stream),
                           'kgdet_image_preprocess')

    def aug_job_tables(self, srcs, plans, flips, dsts, aug_plans):
        """``job_tables`` for ``kgdet_image_preprocess_aug``: ``kgdet_preproc_aug_job`` arrays of at most PREPROC_AUG_MAX_JOBS
        jobs; ``plans`` the size plans of the virtual images, ``aug_plans`` an ``AugPlan`` or ``None`` per job"""
        from . import _lib
        tables = []
        for lo in range(0, len(srcs), _lib.PREPROC_AUG_MAX_JOBS):
            hi = min(len(srcs), lo + _lib.PREPROC_AUG_MAX_JOBS)
            jobs = (_lib.PreprocAugJob * (hi - lo))()
            for k in range(lo, hi):
                s, d, (new_h, new_w, _, _, _), aug = srcs[k], dsts[k], plans[k], aug_plans[k]
                assert s.is_cuda and s.dtype == torch.uint8 and s.stride(2) == 1 and s.stride(1) == 3
                assert d.is_cuda and d.dtype == torch.float32 and d.dim() == 3 and d.shape[0] == 3 and d.stride(2) == 1
                if aug is None:
                    (vh, vw), (oy, ox), numbers = (s.shape[0], s.shape[1]), (0, 0), (0, 0.0, 0.0, 0.0, 0.0, 0 | 1 << 2 | 2 << 4)
                else:
                    if (aug.h, aug.w) != (s.shape[0], s.shape[1]):
                        raise ValueError('job %d: the plan was drawn for a %d x %d image, the raw image is %d x %d'
                                         % (k, aug.h, aug.w, s.shape[0], s.shape[1]))
                    (vh, vw), (oy, ox), numbers = aug.virtual_hw, aug.origin, aug_job_numbers(aug)
                flags, delta, alpha, sat, hue, perm = numbers
                fill = aug_fill(aug, self.mean, self.to_rgb)
                jobs[k - lo] = _lib.PreprocAugJob(
                    s.data_ptr(), s.shape[0], s.shape[1], s.stride(0), d.data_ptr(), d.stride(0), d.stride(1),
                    int(new_h), int(new_w), d.shape[1], d.shape[2], float(axis_scale(vh, new_h)),
                    float(axis_scale(vw, new_w)), 1 if flips[k] else 0, int(vh), int(vw), int(oy), int(ox),
                    (ctypes.c_float * 3)(*[float(x) for x in fill]), float(delta), float(alpha), float(sat), float(hue),
                    int(perm), int(flags))
            tables.append(jobs)
        return tables

    def launch_aug_tables(self, tables):
        """one ``kgdet_image_preprocess_aug`` launch per table on the device's current stream"""
        from . import _lib
        L = _lib.lib()
        fp = ctypes.POINTER(ctypes.c_float)
        mean, std = np.ascontiguousarray(self.mean, dtype=np.float32), np.ascontiguousarray(self.std, dtype=np.float32)
        with torch.cuda.device(self.device):
            stream = _lib.current_stream()
            for jobs in tables:
                _lib.check(L.kgdet_image_preprocess_aug(jobs, ctypes.c_int32(len(jobs)), mean.ctypes.data_as(fp),
                                                        std.ctypes.data_as(fp), ctypes.c_int32(0 if self.to_rgb else 1),
                                                        stream), 'kgdet_image_preprocess_aug')

    def _launch(self, srcs, plans, flips, dsts, aug_plans=None):
        if aug_plans is None:
            self.launch_tables(self.job_tables(srcs, plans, flips, dsts))
        else:
            self.launch_aug_tables(self.aug_job_tables(srcs, plans, flips, dsts, aug_plans))

    def _prepare(self, raws, scales, flips, keep_ratio, aug_plans=None):
        """-> (device sources, size plans, metas, aug_plans or None when every entry is None)"""
        if not (len(raws) == len(scales) == len(flips)):
            raise ValueError('one scale and one flip per raw image')
        if aug_plans is not None and len(aug_plans) != len(raws):
            raise ValueError('one augmentation plan (or None) per raw image')
        if aug_plans is None or all(a is None for a in aug_plans):
            aug_plans = None
            plans = [self.plan(r, s, keep_ratio) for r, s in zip(raws, scales)]
        else:
            sizes = [tuple(r.shape[:2]) if a is None else a.virtual_hw for r, a in zip(raws, aug_plans)]
            plans = [plan(vh, vw, s, keep_ratio, self.size_divisor) for (vh, vw), s in zip(sizes, scales)]
        return self._upload(raws), plans, [(p[2], p[3], p[4]) for p in plans], aug_plans

    def __call__(self, raws, scales, flips, keep_ratio=True, out=None, common_size=None, aug_plans=None):
        srcs, plans, metas, aug_plans = self._prepare(raws, scales, flips, keep_ratio, aug_plans)
        B = len(raws)
        pads = [(p[3][0], p[3][1]) for p in plans]
        if common_size is None:
            if len(set(pads)) > 1:
                raise ValueError('the images pad to different shapes %s: pass common_size' % sorted(set(pads)))
            H, W = pads[0] if pads else (0, 0)
        elif common_size is True:
            H, W = max(p[0] for p in pads), max(p[1] for p in pads)
        else:
            H, W = common_size
            if any(p[0] > H or p[1] > W for p in pads):
                raise ValueError('common_size %s does not hold pad shapes %s' % ((H, W), sorted(set(pads))))
        if out is None:
            out = torch.empty((B, 3, H, W), dtype=torch.float32, device=self.device)
        elif (not out.is_cuda or out.device != self.device or out.dtype != torch.float32 or tuple(out.shape) != (B, 3, H, W)
              or out.stride(3) != 1):
            raise ValueError('out must be a cuda float32 [%d, 3, %d, %d] tensor on %s with a contiguous last dimension'
                             % (B, H, W, self.device))
        self._launch(srcs, plans, flips, [out[b] for b in range(B)], aug_plans)
        return out, metas

    def separate(self, raws, scales, flips, keep_ratio=True, aug_plans=None):
        """-> ([1, 3, H_a, W_a] per job, metas): every job at its own ``pad_shape``, one allocation, one launch"""
        srcs, plans, metas, aug_plans = self._prepare(raws, scales, flips, keep_ratio, aug_plans)
        sizes = [3 * p[3][0] * p[3][1] for p in plans]
        offs, total = [], 0
        for s in sizes:
            offs.append(total)
            total += (s + 3) // 4 * 4                 # (every slot starts on a 16-byte boundary)
        flat = torch.empty(total, dtype=torch.float32, device=self.device)
        outs = [flat[o:o + s].view(1, 3, p[3][0], p[3][1]) for o, s, p in zip(offs, sizes, plans)]
        self._launch(srcs, plans, flips, [t[0] for t in outs], aug_plans)
        return outs, metas
