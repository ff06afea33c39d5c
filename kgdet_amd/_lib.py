"""ctypes binding of libkgdet_hip.so (include/kgdet_hip.h).

The HIP library IS the product: there is no CPU or pure-PyTorch fallback behind it.  If the
shared object is missing or an entry point fails, the caller gets an exception.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('KGDET_LIB') or os.path.join(_HERE, 'libkgdet_hip.so')   # KGDET_LIB: experiment builds
CSRC = os.path.join(_HERE, 'csrc')

KGDET_OK = 0
KGDET_E_SHAPE = 1
KGDET_E_WORKSPACE = 2
KGDET_E_HIP = 3
KGDET_E_UNSUPPORTED = 4
KGDET_E_PARTIAL = 5

DCN_RELU = 1
DCN_BF16 = 2         # forward operands rounded to bf16 once (autocast inference)
DCN_EXACT_FP32 = 4   # forward on the exact-fp32 MFMA kernel instead of the bf16 hi/lo split


class DcnShape(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        'N', 'C', 'H', 'W', 'O', 'kh', 'kw', 'stride_h', 'stride_w', 'pad_h', 'pad_w', 'dil_h',
        'dil_w', 'groups', 'deformable_groups', 'out_channel_offset', 'out_channels_total')]


class PsroiShape(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        'B', 'C', 'H', 'W', 'R', 'out_dim', 'group_size', 'pooled_size', 'part_size',
        'sample_per_part', 'no_trans', 'num_classes')] + [
        ('spatial_scale', ctypes.c_float), ('trans_std', ctypes.c_float)]


class AugSegment(ctypes.Structure):
    """kgdet_aug_segment (one test-time augmentation's decoded candidates)"""
    _fields_ = [('boxes', ctypes.c_void_p), ('scores', ctypes.c_void_p), ('kpts', ctypes.c_void_p), ('n', ctypes.c_int64),
                ('img_w', ctypes.c_float), ('scale', ctypes.c_double), ('flip', ctypes.c_int32)]


PREPROC_MAX_JOBS = 32   # KGDET_PREPROC_MAX_JOBS
COCO_ACC_TILE = 1024    # KGDET_COCO_ACC_TILE: positions of a category's sequence per scan tile
COCO_PACK_ROWS = 4      # KGDET_COCO_PACK_ROWS: landmark rows (waves) per workgroup
COCO_ORDER_MAX_ROWS = 1024    # KGDET_COCO_ORDER_MAX_ROWS: detections per image kgdet_coco_order_dets ranks in LDS
COCO_ORDER_MAX_LABELS = 64    # KGDET_COCO_ORDER_MAX_LABELS
COCO_JSON_MAX_K = 1024        # KGDET_COCO_JSON_MAX_K: landmarks of a record kgdet_coco_json_write assembles in LDS
DRAW_MAX_IMAGES, DRAW_MAX_ROWS, DRAW_MAX_K, DRAW_MAX_LABELS = 32, 1024, 1024, 64    # KGDET_DRAW_MAX_*: kgdet_draw_detections
JPEG_MAX_IMAGES, JPEG_RANGE_BYTES = 32, 4096    # KGDET_JPEG_*: kgdet_jpeg_encode (jpeg.py carries the same numbers)
JPEG_DECODE_MAX_IMAGES, JPEG_DECODE_SUBSEQ_BITS, JPEG_DECODE_CHUNK_LANES, JPEG_DECODE_TABLE_BYTES = 32, 512, 1024, 1024   # KGDET_JPEG_DECODE_*


class JpegDecodeJob(ctypes.Structure):
    """kgdet_jpeg_decode_job (one file's scan and table block inside the source buffer -> one picture of the output buffer)"""
    _fields_ = [(n, ctypes.c_int64) for n in ('scan_offset', 'scan_bytes', 'tables_offset', 'dst_offset')] + [
        (n, ctypes.c_int32) for n in ('H', 'W', 'mode', 'reserved')]


class CocoPackedDets(ctypes.Structure):
    """kgdet_coco_packed_dets (the packed arrays of one result kind, device pointers)"""
    _fields_ = [('n', ctypes.c_int64)] + [(n, ctypes.c_void_p) for n in (
        'cell', 'img_idx', 'cat_idx', 'id', 'score', 'bbox', 'area', 'kxy32')]


class PreprocJob(ctypes.Structure):
    """kgdet_preproc_job (one raw image -> one [3, out_h, out_w] slot of the detector's input)"""
    _fields_ = [('src', ctypes.c_void_p), ('src_h', ctypes.c_int32), ('src_w', ctypes.c_int32),
                ('src_row_bytes', ctypes.c_int32), ('dst', ctypes.c_void_p), ('dst_channel_stride', ctypes.c_int64),
                ('dst_row_stride', ctypes.c_int32), ('new_h', ctypes.c_int32), ('new_w', ctypes.c_int32),
                ('out_h', ctypes.c_int32), ('out_w', ctypes.c_int32), ('scale_y', ctypes.c_float),
                ('scale_x', ctypes.c_float), ('flip', ctypes.c_int32)]


PREPROC_AUG_MAX_JOBS = 16   # KGDET_PREPROC_AUG_MAX_JOBS
AUG_COLOUR, AUG_BRIGHTNESS, AUG_CONTRAST, AUG_CONTRAST_FIRST, AUG_SATURATION, AUG_HUE, AUG_PERMUTE = 1, 2, 4, 8, 16, 32, 64


class PreprocAugJob(ctypes.Structure):
    """kgdet_preproc_aug_job (kgdet_preproc_job + the expand / crop window and the photometric distortion of one image)"""
    _fields_ = PreprocJob._fields_ + [
        ('vh', ctypes.c_int32), ('vw', ctypes.c_int32), ('oy', ctypes.c_int32), ('ox', ctypes.c_int32),
        ('fill', ctypes.c_float * 3), ('delta', ctypes.c_float), ('alpha', ctypes.c_float), ('sat', ctypes.c_float),
        ('hue', ctypes.c_float), ('perm', ctypes.c_int32), ('flags', ctypes.c_uint32)]


def build(force=False):
    """Compile every HIP source for gfx950 into kgdet_amd/libkgdet_hip.so (hipcc, in-tree)."""
    cmd = ['make', '-C', CSRC, '-j8']
    if force:
        cmd.append('-B')
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None


def lib():
    """The loaded library.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                'kgdet_amd: %s is missing -- run `python -c "import __graft_entry__ as g; g.build()"` '
                'or `make -C kgdet_amd/csrc`. There is no non-HIP fallback.' % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.kgdet_last_error.restype = ctypes.c_char_p
        for name in ('kgdet_dcn_packed_weight_bytes', 'kgdet_dcn_workspace_bytes', 'kgdet_dcn_group_workspace_bytes',
                     'kgdet_nms_workspace_bytes', 'kgdet_deform_psroi_backward_workspace_bytes',
                     'kgdet_deform_psroi_forward_workspace_bytes', 'kgdet_head_loss_workspace_bytes', 'kgdet_serial_loss_workspace_bytes',
                     'kgdet_moment_bbox_backward_workspace_bytes', 'kgdet_multiclass_soft_nms_workspace_bytes'):
            if hasattr(L, name):
                getattr(L, name).restype = ctypes.c_size_t
        for name in ('kgdet_multiclass_soft_nms_supported', 'kgdet_multiclass_nms_supported'):
            if hasattr(L, name):
                getattr(L, name).restype = ctypes.c_int
                getattr(L, name).argtypes = [ctypes.c_int32] * 4
        if hasattr(L, 'kgdet_coco_similarity'):      # evaluation_device.py: int64 sizes among the arguments
            vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
            L.kgdet_coco_similarity.restype = L.kgdet_coco_match.restype = ctypes.c_int
            L.kgdet_coco_similarity.argtypes = [i32, vp, vp, i32, i64, i64, i64] + [vp] * 8 + [i32, vp, vp]
            L.kgdet_coco_match.argtypes = [vp, vp, i32, i64, i64, i64] + [vp] * 6 + [i32, vp, i32] + [vp] * 5
        if hasattr(L, 'kgdet_coco_accumulate'):
            vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
            L.kgdet_coco_count_gt.restype = L.kgdet_coco_accumulate.restype = L.kgdet_coco_pack_landmarks.restype = ctypes.c_int
            L.kgdet_coco_count_gt.argtypes = [vp, vp, i64, i32, i32, vp, vp]
            L.kgdet_coco_accumulate.argtypes = [vp] * 9 + [i64] + [i32] * 5 + [i64] + [vp] * 4 + [ctypes.c_size_t, vp]
            L.kgdet_coco_pack_landmarks.argtypes = [vp, i64, i32, i32, vp, vp, vp, vp]
        if hasattr(L, 'kgdet_coco_order_dets'):
            vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
            L.kgdet_coco_order_dets.restype = L.kgdet_coco_scatter_dets.restype = ctypes.c_int
            L.kgdet_coco_order_dets.argtypes = [vp, i64, i32, i32, vp, vp, i32, i32, i64, i32, i32, i32] + [vp] * 7
            L.kgdet_coco_scatter_dets.argtypes = ([vp, i64, i32, i32, vp, i32, i64] + [vp] * 5 + [i32, i32]
                                                  + [ctypes.POINTER(CocoPackedDets)] * 2 + [vp, vp])
        if hasattr(L, 'kgdet_coco_json_write'):
            vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
            L.kgdet_coco_json_measure.restype = L.kgdet_coco_json_write.restype = ctypes.c_int
            L.kgdet_coco_json_measure.argtypes = [vp, i64, i32, i32] + [vp] * 5 + [i32, i32, vp, vp, vp, i64, vp, vp]
            L.kgdet_coco_json_write.argtypes = [i32, vp, i64, i32, i32] + [vp] * 5 + [i32, i32, i64, i64, i64, vp, i64, vp, vp]
        if hasattr(L, 'kgdet_draw_detections'):      # visualize.py: host tables, int64 sizes and a float among the arguments
            vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
            L.kgdet_draw_detections.restype = ctypes.c_int
            L.kgdet_draw_detections.argtypes = ([vp, i64, vp, i64, vp, vp, i32, vp, i64, i32, i32, vp, i32, vp, vp, i32, vp, vp,
                                                 ctypes.c_float] + [i32] * 6 + [vp])
        if hasattr(L, 'kgdet_jpeg_encode'):          # jpeg.py: host tables, int64 and size_t sizes among the arguments
            vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
            L.kgdet_jpeg_workspace_bytes.restype = ctypes.c_size_t
            L.kgdet_jpeg_workspace_bytes.argtypes = [vp, i32]
            L.kgdet_jpeg_encode.restype = L.kgdet_jpeg_write.restype = ctypes.c_int
            L.kgdet_jpeg_encode.argtypes = [vp, i64, vp, i32, i32, vp, ctypes.c_size_t, vp, vp]
            L.kgdet_jpeg_write.argtypes = [vp, i32, i32, vp, ctypes.c_size_t, vp, vp, i64, vp, vp]
        if hasattr(L, 'kgdet_jpeg_decode'):          # jpeg.py: a host job table, int64 and size_t sizes among the arguments
            vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
            L.kgdet_jpeg_decode_workspace_bytes.restype = ctypes.c_size_t
            L.kgdet_jpeg_decode_workspace_bytes.argtypes = [vp, i32]
            L.kgdet_jpeg_decode.restype = ctypes.c_int
            L.kgdet_jpeg_decode.argtypes = [vp, i64, vp, i32, vp, ctypes.c_size_t, vp, i64, vp, vp]
            L.kgdet_jpeg_decode_stages.restype = ctypes.c_int
            L.kgdet_jpeg_decode_stages.argtypes = L.kgdet_jpeg_decode.argtypes + [i32]
        if hasattr(L, 'kgdet_jpeg_decode_camera'):   # the same signatures: 4:2:2 files and restart intervals
            L.kgdet_jpeg_decode_camera_workspace_bytes.restype = ctypes.c_size_t
            L.kgdet_jpeg_decode_camera_workspace_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int32]
            L.kgdet_jpeg_decode_camera.restype = ctypes.c_int
            L.kgdet_jpeg_decode_camera.argtypes = L.kgdet_jpeg_decode.argtypes
            L.kgdet_jpeg_decode_camera_stages.restype = ctypes.c_int
            L.kgdet_jpeg_decode_camera_stages.argtypes = L.kgdet_jpeg_decode_stages.argtypes
        _lib = L
    return _lib


def check(rc, what=''):
    """Map a status code to the exception the reference raises for the same condition."""
    if rc == KGDET_OK:
        return
    msg = lib().kgdet_last_error().decode('utf-8', 'replace')
    if rc == KGDET_E_UNSUPPORTED:
        raise NotImplementedError('%s: %s' % (what, msg))
    raise RuntimeError('%s: %s' % (what, msg))


def ptr(t):
    """device pointer of a tensor (or NULL for None)"""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def raw_stream(device_index=None):
    """the current HIP stream of the device as an integer handle.  torch.cuda.current_stream() costs ~9 us of Python
    per call (a training step makes ~400 of them); the raw getter is a single C call."""
    import torch
    if device_index is None:
        device_index = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(device_index)


def current_stream():
    return ctypes.c_void_p(raw_stream())
