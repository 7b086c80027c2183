"""Thin ctypes binding of libpicsong_hip.so (include/picsong_hip.h) for tests and bench.py.

PyTorch is used only as plumbing: device memory (torch tensors -> raw pointers) and the HIP stream.
There is NO fallback: if the shared library is missing or no GPU is present this module raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
SO_PATH = os.environ.get("PICSONG_SO", os.path.join(PKG, "csrc", "libpicsong_hip.so"))

PICSONG_OK = 0
PICSONG_ERR_RATE = -7
PICSONG_ERR_QUALITY = -8


class Params(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("wl", C.c_int), ("cp", C.c_int),
                ("lossy", C.c_int), ("qs", C.c_float), ("k", C.c_float), ("cb_width", C.c_int),
                ("cb_height", C.c_int), ("bit_depth", C.c_int), ("frames", C.c_int),
                ("components", C.c_int), ("is_rgb", C.c_int)]


class Image(C.Structure):
    """picsong_image: W x H pixels (the context's) on the device at a byte pitch, in one of the LAYOUT_* layouts."""
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_size_t), ("plane_stride", C.c_size_t), ("layout", C.c_int)]


LAYOUT_GREY8, LAYOUT_PLANAR3, LAYOUT_RGB24, LAYOUT_BGR24, LAYOUT_RGBA32, LAYOUT_BGRA32, LAYOUT_GREY16 = range(7)
LAYOUT_PLANAR3_16, LAYOUT_RGB48, LAYOUT_RGBA64 = 7, 8, 9          # deep RGB contexts: native uint16 samples
LAYOUT_BPP = (1, 1, 3, 3, 4, 4, 2, 2, 6, 8)
LAYOUTS_16 = (LAYOUT_GREY16, LAYOUT_PLANAR3_16, LAYOUT_RGB48, LAYOUT_RGBA64)


class LutInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n_bitplanes", "n_subbands", "ctx_ref", "ctx_sign", "ctx_sig",
                                       "precision", "n_files", "n_bp_files", "n_ref", "n_sig", "n_sign",
                                       "n_tables", "cp")]


EXPORTS = [
    "picsong_last_error", "picsong_version", "picsong_pad_dim", "picsong_dwt_extra",
    "picsong_max_stream_shorts", "picsong_header_pack", "picsong_header_unpack", "picsong_lut_load",
    "picsong_lut_load_k",
    "picsong_ctx_create", "picsong_ctx_destroy", "picsong_ctx_set_lut", "picsong_ctx_padded_dims",
    "picsong_ctx_set_pipelined",
    "picsong_level_shift_fwd", "picsong_level_shift_inv", "picsong_dwt_forward", "picsong_dwt_inverse",
    "picsong_dwt_forward_u8", "picsong_bpc_encode", "picsong_bpc_decode", "picsong_bitstream_pack",
    "picsong_bitstream_unpack", "picsong_last_total", "picsong_encode_frame", "picsong_decode_frame",
    "picsong_pad_frame_host", "picsong_range_flag", "picsong_profile_begin", "picsong_profile_read",
    "picsong_encode_frame_stripe", "picsong_ctx_set_lut_component", "picsong_rgb_forward", "picsong_rgb_inverse",
    "picsong_encode_plane", "picsong_decode_plane",
    "picsong_ctx_set_lut_device", "picsong_bpc_encode_component", "picsong_bpc_decode_component",
    "picsong_encode_frames", "picsong_last_totals", "picsong_selftest_lds_order",
    "picsong_dwt_forward_band", "picsong_dwt_forward_tail", "picsong_encode_stripe_coded", "picsong_lut_load_cp",
    "picsong_copy_last_totals", "picsong_decode_frames", "picsong_encode_rgb_frame", "picsong_decode_rgb_frame",
    "picsong_reduced_dims", "picsong_decode_frame_reduced", "picsong_decode_frames_reduced",
    "picsong_decode_rgb_frame_reduced",
    "picsong_window_codeblocks", "picsong_decode_frame_window", "picsong_decode_frames_window",
    "picsong_decode_rgb_frame_window",
    "picsong_train_begin", "picsong_train_info", "picsong_train_reset", "picsong_train_end", "picsong_train_coeffs",
    "picsong_train_frames", "picsong_train_rgb_frame", "picsong_train_counts", "picsong_lut_from_counts",
    "picsong_lut_save",
    "picsong_rate_qs", "picsong_ctx_set_qs", "picsong_encode_frame_rate", "picsong_encode_frames_rate",
    "picsong_encode_rgb_frame_rate",
    "picsong_psnr_to_sse", "picsong_sse_to_psnr", "picsong_frames_sse", "picsong_encode_frame_quality",
    "picsong_encode_frames_quality", "picsong_encode_rgb_frame_quality",
    "picsong_ingest_frames", "picsong_emit_frames", "picsong_encode_images", "picsong_decode_images",
    "picsong_encode_rgb_image", "picsong_decode_rgb_image",
    "picsong_encode_rgb_frames", "picsong_decode_rgb_frames", "picsong_encode_rgb_images", "picsong_decode_rgb_images",
    "picsong_decode_rgb_frames_reduced", "picsong_decode_rgb_frames_window", "picsong_decode_rgb_images_reduced",
    "picsong_decode_rgb_images_window",
    "picsong_encode_rgb_frames_rate", "picsong_encode_rgb_frames_quality", "picsong_train_rgb_frames",
    "picsong_ctx_set_decode_drop", "picsong_ctx_get_decode_drop", "picsong_drop_planes",
    "picsong_depth_range_guaranteed", "picsong_pad_frame16_host", "picsong_level_shift_fwd16", "picsong_dwt_forward_u16",
    "picsong_encode_frames16", "picsong_decode_frames16",
    "picsong_depth_range_guaranteed_rgb", "picsong_rgb_forward16", "picsong_rgb_inverse16",
    "picsong_encode_rgb_frames16", "picsong_decode_rgb_frames16",
    "picsong_decode_frames16_reduced", "picsong_decode_frames16_window", "picsong_decode_rgb_frames16_reduced",
    "picsong_decode_rgb_frames16_window",
    "picsong_ssim_windows", "picsong_ssim_to_dssim", "picsong_dssim_to_ssim", "picsong_frames_dssim",
    "picsong_encode_frame_ssim", "picsong_encode_frames_ssim", "picsong_encode_rgb_frames_ssim",
]

_lib = None


def load():
    """Load the HIP library; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: its wheel bundles a HIP runtime that it exposes process-wide; loading it before
    # libpicsong_hip.so makes the library bind to that same runtime, so the device pointers and
    # hipStream_t handles torch hands out are valid inside the library (one runtime per process).
    import torch  # noqa: F401
    if not os.path.exists(SO_PATH):
        raise RuntimeError(f"{SO_PATH} not built: run __graft_entry__.build() (hipcc, gfx950). "
                           "There is no CPU fallback.")
    L = C.CDLL(SO_PATH)
    vp, i = C.c_void_p, C.c_int
    L.picsong_last_error.restype = C.c_char_p
    L.picsong_version.restype = C.c_char_p
    L.picsong_pad_dim.argtypes = [i]
    L.picsong_dwt_extra.restype = C.c_size_t
    L.picsong_dwt_extra.argtypes = [i, i, i]
    L.picsong_max_stream_shorts.restype = C.c_size_t
    L.picsong_max_stream_shorts.argtypes = [i, i]
    L.picsong_header_pack.argtypes = [C.POINTER(Params), vp]
    L.picsong_header_unpack.argtypes = [vp, C.POINTER(Params)]
    L.picsong_lut_load.argtypes = [C.c_char_p, i, i, i, C.POINTER(LutInfo), vp, C.c_size_t]
    L.picsong_lut_load_k.argtypes = [C.c_char_p, i, i, i, i, C.POINTER(LutInfo), vp, C.c_size_t]
    L.picsong_ctx_create.argtypes = [C.POINTER(Params), i, C.POINTER(vp)]
    L.picsong_ctx_destroy.argtypes = [vp]
    L.picsong_ctx_destroy.restype = None
    L.picsong_ctx_set_lut.argtypes = [vp, C.POINTER(LutInfo), vp]
    L.picsong_ctx_padded_dims.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    L.picsong_ctx_set_pipelined.argtypes = [vp, i]
    L.picsong_level_shift_fwd.argtypes = [vp, vp, vp, vp]
    L.picsong_level_shift_inv.argtypes = [vp, vp, vp]
    L.picsong_dwt_forward.argtypes = [vp, vp, vp, vp]
    L.picsong_dwt_forward_u8.argtypes = [vp, vp, vp, vp]
    L.picsong_dwt_inverse.argtypes = [vp, vp, vp, vp]
    L.picsong_bpc_encode.argtypes = [vp, vp, vp, vp, vp]
    L.picsong_bpc_decode.argtypes = [vp, vp, vp, vp, vp]
    L.picsong_bitstream_pack.argtypes = [vp, vp, vp, vp, vp, C.POINTER(i), vp]
    L.picsong_bitstream_unpack.argtypes = [vp, vp, vp, vp, vp]
    L.picsong_last_total.argtypes = [vp, vp, C.POINTER(i)]
    L.picsong_encode_frame.argtypes = [vp, vp, i, vp, vp]
    L.picsong_decode_frame.argtypes = [vp, vp, vp, vp]
    L.picsong_encode_frame_stripe.argtypes = [vp, vp, i, i, vp, vp]
    L.picsong_ctx_set_lut_component.argtypes = [vp, i, C.POINTER(LutInfo), vp]
    L.picsong_rgb_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.picsong_rgb_inverse.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.picsong_encode_plane.argtypes = [vp, vp, i, i, vp, vp]
    L.picsong_decode_plane.argtypes = [vp, vp, i, vp, vp]
    L.picsong_pad_frame_host.argtypes = [vp, i, i, vp, i, i]
    L.picsong_range_flag.argtypes = [vp, vp, C.POINTER(i)]
    L.picsong_profile_begin.argtypes = [vp, i]
    L.picsong_profile_read.argtypes = [vp, C.POINTER(i), vp, i]
    if hasattr(L, "picsong_encode_frames"):          # (A/B runs load older variant libraries through PICSONG_SO)
        L.picsong_encode_frames.argtypes = [vp, i, vp, C.c_size_t, i, vp, C.c_size_t, vp]
        L.picsong_last_totals.argtypes = [vp, vp, i, C.POINTER(i)]
        L.picsong_ctx_set_lut_device.argtypes = [vp, i, C.POINTER(LutInfo), vp]
        L.picsong_bpc_encode_component.argtypes = [vp, i, vp, vp, vp, vp]
        L.picsong_bpc_decode_component.argtypes = [vp, i, vp, vp, vp, vp]
    if hasattr(L, "picsong_copy_last_totals"):
        L.picsong_copy_last_totals.argtypes = [vp, vp, i, vp]
    if hasattr(L, "picsong_decode_frames"):
        L.picsong_decode_frames.argtypes = [vp, i, vp, C.c_size_t, vp, C.c_size_t, vp]
    if hasattr(L, "picsong_encode_rgb_frame"):
        L.picsong_encode_rgb_frame.argtypes = [vp, vp, vp, vp, i, vp, C.c_size_t, vp]
        L.picsong_decode_rgb_frame.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, vp]
    if hasattr(L, "picsong_reduced_dims"):
        L.picsong_reduced_dims.argtypes = [vp, i] + [C.POINTER(i)] * 5
        L.picsong_decode_frame_reduced.argtypes = [vp, vp, i, vp, vp]
        L.picsong_decode_frames_reduced.argtypes = [vp, i, vp, C.c_size_t, i, vp, C.c_size_t, vp]
        L.picsong_decode_rgb_frame_reduced.argtypes = [vp, vp, C.c_size_t, i, vp, vp, vp, vp]
    if hasattr(L, "picsong_window_codeblocks"):
        L.picsong_window_codeblocks.argtypes = [vp, i, i, i, i, i, C.POINTER(i)]
        L.picsong_decode_frame_window.argtypes = [vp, vp, i, i, i, i, i, vp, C.c_size_t, vp]
        L.picsong_decode_frames_window.argtypes = [vp, i, vp, C.c_size_t, i, i, i, i, i, vp, C.c_size_t, C.c_size_t, vp]
        L.picsong_decode_rgb_frame_window.argtypes = [vp, vp, C.c_size_t, i, i, i, i, i, vp, vp, vp, C.c_size_t, vp]
    if hasattr(L, "picsong_lut_load_cp"):
        L.picsong_lut_load_cp.argtypes = [C.c_char_p, i, i, i, i, C.POINTER(LutInfo), vp, C.c_size_t]
    if hasattr(L, "picsong_dwt_forward_band"):
        L.picsong_dwt_forward_band.argtypes = [vp, vp, i, i, vp, vp]
        L.picsong_dwt_forward_tail.argtypes = [vp, vp, vp]
        L.picsong_encode_stripe_coded.argtypes = [vp, vp, i, i, vp, vp]
    if hasattr(L, "picsong_train_begin"):
        L.picsong_train_begin.argtypes = [vp, C.POINTER(LutInfo)]
        L.picsong_train_info.argtypes = [vp, C.POINTER(LutInfo)]
        L.picsong_train_reset.argtypes = [vp]
        L.picsong_train_end.argtypes = [vp]
        L.picsong_train_coeffs.argtypes = [vp, i, vp, vp]
        L.picsong_train_frames.argtypes = [vp, i, vp, C.c_size_t, vp]
        L.picsong_train_rgb_frame.argtypes = [vp, vp, vp, vp, vp]
        L.picsong_train_counts.argtypes = [vp, i, vp, vp, C.c_size_t]
        L.picsong_lut_from_counts.argtypes = [C.POINTER(LutInfo), vp, vp, vp]
        L.picsong_lut_save.argtypes = [C.c_char_p, i, C.POINTER(LutInfo), i, vp]
    if hasattr(L, "picsong_rate_qs"):
        L.picsong_rate_qs.argtypes = [i, C.POINTER(C.c_float)]
        L.picsong_ctx_set_qs.argtypes = [vp, C.c_float]
        L.picsong_encode_frame_rate.argtypes = [vp, vp, i, C.c_size_t, i, i, vp, vp, C.POINTER(i), C.POINTER(i)]
        L.picsong_encode_frames_rate.argtypes = [vp, i, vp, C.c_size_t, i, C.c_size_t, i, i, vp, C.c_size_t, vp,
                                                 C.POINTER(i), C.POINTER(i)]
        L.picsong_encode_rgb_frame_rate.argtypes = [vp, vp, vp, vp, i, C.c_size_t, i, i, vp, C.c_size_t, vp,
                                                    C.POINTER(i), C.POINTER(i)]
    if hasattr(L, "picsong_frames_sse"):
        u64 = C.c_uint64
        L.picsong_psnr_to_sse.argtypes = [C.c_double, u64, C.POINTER(u64)]
        L.picsong_sse_to_psnr.argtypes = [u64, u64, C.POINTER(C.c_double)]
        L.picsong_frames_sse.argtypes = [vp, i, vp, C.c_size_t, vp, C.c_size_t, vp, vp]
        L.picsong_encode_frame_quality.argtypes = [vp, vp, i, u64, i, i, vp, vp, C.POINTER(i), C.POINTER(i), C.POINTER(u64)]
        L.picsong_encode_frames_quality.argtypes = [vp, i, vp, C.c_size_t, i, u64, i, i, vp, C.c_size_t, vp,
                                                    C.POINTER(i), C.POINTER(i), C.POINTER(u64)]
        L.picsong_encode_rgb_frame_quality.argtypes = [vp, vp, vp, vp, i, u64, i, i, vp, C.c_size_t, vp,
                                                       C.POINTER(i), C.POINTER(i), C.POINTER(u64)]
    if hasattr(L, "picsong_ingest_frames"):
        img = C.POINTER(Image)
        L.picsong_ingest_frames.argtypes = [vp, i, img, C.c_size_t, vp, C.c_size_t, vp]
        L.picsong_emit_frames.argtypes = [vp, i, vp, C.c_size_t, img, C.c_size_t, vp]
        L.picsong_encode_images.argtypes = [vp, i, img, C.c_size_t, i, vp, C.c_size_t, vp]
        L.picsong_decode_images.argtypes = [vp, i, vp, C.c_size_t, img, C.c_size_t, vp]
        L.picsong_encode_rgb_image.argtypes = [vp, img, i, vp, C.c_size_t, vp]
        L.picsong_decode_rgb_image.argtypes = [vp, vp, C.c_size_t, img, vp]
        L.picsong_encode_rgb_frames.argtypes = [vp, i, vp, vp, vp, C.c_size_t, i, i, vp, C.c_size_t, vp]
        L.picsong_decode_rgb_frames.argtypes = [vp, i, vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp]
        L.picsong_encode_rgb_images.argtypes = [vp, i, img, C.c_size_t, i, i, vp, C.c_size_t, vp]
        L.picsong_decode_rgb_images.argtypes = [vp, i, vp, C.c_size_t, img, C.c_size_t, vp]
    if hasattr(L, "picsong_decode_rgb_frames_reduced"):
        img = C.POINTER(Image)
        L.picsong_decode_rgb_frames_reduced.argtypes = [vp, i, vp, C.c_size_t, i, vp, vp, vp, C.c_size_t, vp]
        L.picsong_decode_rgb_frames_window.argtypes = [vp, i, vp, C.c_size_t, i, i, i, i, i, vp, vp, vp, C.c_size_t, C.c_size_t, vp]
        L.picsong_decode_rgb_images_reduced.argtypes = [vp, i, vp, C.c_size_t, i, img, C.c_size_t, vp]
        L.picsong_decode_rgb_images_window.argtypes = [vp, i, vp, C.c_size_t, i, i, i, i, i, img, C.c_size_t, vp]
    if hasattr(L, "picsong_encode_rgb_frames_rate"):
        u64 = C.c_uint64
        L.picsong_encode_rgb_frames_rate.argtypes = [vp, i, vp, vp, vp, C.c_size_t, i, i, C.c_size_t, i, i, vp, C.c_size_t, vp,
                                                     C.POINTER(i), C.POINTER(i)]
        L.picsong_encode_rgb_frames_quality.argtypes = [vp, i, vp, vp, vp, C.c_size_t, i, i, u64, i, i, vp, C.c_size_t, vp,
                                                        C.POINTER(i), C.POINTER(i), C.POINTER(u64)]
        L.picsong_train_rgb_frames.argtypes = [vp, i, vp, vp, vp, C.c_size_t, vp]
    if hasattr(L, "picsong_ctx_set_decode_drop"):
        L.picsong_ctx_set_decode_drop.argtypes = [vp, i]
        L.picsong_ctx_get_decode_drop.argtypes = [vp, C.POINTER(i)]
        L.picsong_drop_planes.argtypes = [i, i, i, i, i, C.POINTER(i)]
    if hasattr(L, "picsong_encode_frames16"):
        L.picsong_depth_range_guaranteed.argtypes = [i, i, i, C.c_float, C.POINTER(i)]
        L.picsong_pad_frame16_host.argtypes = [vp, i, i, vp, i, i]
        L.picsong_level_shift_fwd16.argtypes = [vp, vp, vp, vp]
        L.picsong_dwt_forward_u16.argtypes = [vp, vp, vp, vp]
        L.picsong_encode_frames16.argtypes = [vp, i, vp, C.c_size_t, i, vp, C.c_size_t, vp]
        L.picsong_decode_frames16.argtypes = [vp, i, vp, C.c_size_t, vp, C.c_size_t, vp]
    if hasattr(L, "picsong_encode_rgb_frames16"):
        L.picsong_depth_range_guaranteed_rgb.argtypes = [i, i, i, C.c_float, C.POINTER(i)]
        L.picsong_rgb_forward16.argtypes = [vp] * 8
        L.picsong_rgb_inverse16.argtypes = [vp] * 8
        L.picsong_encode_rgb_frames16.argtypes = [vp, i, vp, vp, vp, C.c_size_t, i, i, vp, C.c_size_t, vp]
        L.picsong_decode_rgb_frames16.argtypes = [vp, i, vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp]
    if hasattr(L, "picsong_decode_frames16_reduced"):
        L.picsong_decode_frames16_reduced.argtypes = [vp, i, vp, C.c_size_t, i, vp, C.c_size_t, vp]
        L.picsong_decode_frames16_window.argtypes = [vp, i, vp, C.c_size_t, i, i, i, i, i, vp, C.c_size_t, C.c_size_t, vp]
        L.picsong_decode_rgb_frames16_reduced.argtypes = [vp, i, vp, C.c_size_t, i, vp, vp, vp, C.c_size_t, vp]
        L.picsong_decode_rgb_frames16_window.argtypes = [vp, i, vp, C.c_size_t, i, i, i, i, i, vp, vp, vp, C.c_size_t, C.c_size_t, vp]
    if hasattr(L, "picsong_frames_dssim"):
        u64 = C.c_uint64
        L.picsong_ssim_windows.argtypes = [i, i, C.POINTER(u64)]
        L.picsong_ssim_to_dssim.argtypes = [C.c_double, u64, C.POINTER(u64)]
        L.picsong_dssim_to_ssim.argtypes = [u64, u64, C.POINTER(C.c_double)]
        L.picsong_frames_dssim.argtypes = [vp, i, vp, C.c_size_t, vp, C.c_size_t, vp, vp]
        L.picsong_encode_frame_ssim.argtypes = [vp, vp, i, u64, i, i, vp, vp, C.POINTER(i), C.POINTER(i), C.POINTER(u64)]
        L.picsong_encode_frames_ssim.argtypes = [vp, i, vp, C.c_size_t, i, u64, i, i, vp, C.c_size_t, vp,
                                                 C.POINTER(i), C.POINTER(i), C.POINTER(u64)]
        L.picsong_encode_rgb_frames_ssim.argtypes = [vp, i, vp, vp, vp, C.c_size_t, i, i, u64, i, i, vp, C.c_size_t, vp,
                                                     C.POINTER(i), C.POINTER(i), C.POINTER(u64)]
    _lib = L
    return L


class PicsongError(RuntimeError):
    pass


def _check(rc):
    if rc != PICSONG_OK:
        raise PicsongError(f"picsong error {rc}: {load().picsong_last_error().decode()}")


class RateError(PicsongError):
    """No quantiser of the search range meets the target size (PICSONG_ERR_RATE)."""


def _check_rate(rc):
    if rc == PICSONG_ERR_RATE:
        raise RateError(load().picsong_last_error().decode())
    _check(rc)


class QualityError(PicsongError):
    """No quantiser of the search range meets the distortion limit (PICSONG_ERR_QUALITY)."""


def _check_quality(rc):
    if rc == PICSONG_ERR_QUALITY:
        raise QualityError(load().picsong_last_error().decode())
    _check(rc)


def psnr_to_sse(psnr_db, samples):
    """The largest SSE over `samples` 8-bit samples whose PSNR is at least psnr_db (picsong_psnr_to_sse)."""
    v = C.c_uint64()
    _check(load().picsong_psnr_to_sse(psnr_db, samples, C.byref(v)))
    return v.value


def sse_to_psnr(sse, samples):
    """The PSNR (dB) of an SSE over `samples` 8-bit samples; inf for sse = 0 (picsong_sse_to_psnr)."""
    v = C.c_double()
    _check(load().picsong_sse_to_psnr(sse, samples, C.byref(v)))
    return v.value


def ssim_windows(w, h):
    """The 8 x 8 windows (origins 4 x, 4 y) of a w x h plane (picsong_ssim_windows; raises below 8 x 8)."""
    v = C.c_uint64()
    _check(load().picsong_ssim_windows(w, h, C.byref(v)))
    return v.value


def ssim_to_dssim(ssim, windows):
    """The largest DSSIM sum over `windows` windows whose SSIM is at least `ssim` (picsong_ssim_to_dssim)."""
    v = C.c_uint64()
    _check(load().picsong_ssim_to_dssim(ssim, windows, C.byref(v)))
    return v.value


def dssim_to_ssim(dssim, windows):
    """The SSIM of a DSSIM sum over `windows` windows (picsong_dssim_to_ssim)."""
    v = C.c_double()
    _check(load().picsong_dssim_to_ssim(dssim, windows, C.byref(v)))
    return v.value


def rate_qs(j):
    """q(j) = float32(j / 10000.0), the gain a decoder reads for a stored j; raises for a j outside 1..16383 or one the
    header does not store exactly (picsong_rate_qs)."""
    q = C.c_float()
    _check(load().picsong_rate_qs(j, C.byref(q)))
    return q.value


def drop_planes(aw, ah, wl, drop, cb):
    """d(cb) = max(0, drop - level(cb)): the bit-planes raster codeblock `cb` of an aw x ah padded frame of `wl` levels
    leaves undecoded under Codec.set_decode_drop(drop) (picsong_drop_planes; host only)."""
    d = C.c_int()
    _check(load().picsong_drop_planes(aw, ah, wl, drop, cb, C.byref(d)))
    return d.value


def pad_dim(v):
    return load().picsong_pad_dim(v)


def dwt_extra(aw, ah, wl):
    return load().picsong_dwt_extra(aw, ah, wl)


def lut_load(folder, wl, component=1, fill=0, n_tables=1, cp=2):
    """Returns (LutInfo, np.int32 table) parsed by the library's own host parser.
    n_tables = 1: file _0 (k = 0); n_tables = 0: every bit-plane file (the -k > 0 layout);
    cp = 3: the five sections of the 3-coding-pass mode."""
    L = load()
    info = LutInfo()
    if cp == 3:
        _check(L.picsong_lut_load_cp(folder.encode(), component, wl, fill, 3, C.byref(info), None, 0))
        table = np.empty(info.n_ref + 2 * (info.n_sig + info.n_sign), np.int32)
        _check(L.picsong_lut_load_cp(folder.encode(), component, wl, fill, 3, C.byref(info),
                                     table.ctypes.data_as(C.c_void_p), table.size))
        return info, table
    _check(L.picsong_lut_load_k(folder.encode(), component, wl, fill, n_tables, C.byref(info), None, 0))
    table = np.empty((info.n_ref + info.n_sig + info.n_sign) * info.n_tables, np.int32)
    _check(L.picsong_lut_load_k(folder.encode(), component, wl, fill, n_tables, C.byref(info),
                                table.ctypes.data_as(C.c_void_p), table.size))
    return info, table


TRAIN_GEOMETRY = dict(n_bitplanes=15, n_subbands=3, ctx_ref=1, ctx_sign=4, ctx_sig=9, precision=7)   # the shipped folders'


def lut_from_counts(info, counts, prior=None):
    """The table of uint64 counts[entries][2] (picsong_lut_from_counts); `info` complete (Codec.train_info, lut_load)."""
    counts = np.ascontiguousarray(counts, np.uint64)
    n = info.n_ref + info.n_sig + info.n_sign
    assert counts.shape == (n, 2)
    table = np.empty(n, np.int32)
    pp = None
    if prior is not None:
        prior = np.ascontiguousarray(prior, np.int32)
        assert prior.size >= n
        pp = prior.ctypes.data_as(C.c_void_p)
    _check(load().picsong_lut_from_counts(C.byref(info), counts.ctypes.data_as(C.c_void_p), pp,
                                          table.ctypes.data_as(C.c_void_p)))
    return table


def lut_save(folder, component, info, wl, table):
    """Write `table` as a LUT folder's files of `component` (0 un-suffixed, 1/2/3 = R/G/B) for `wl` levels."""
    table = np.ascontiguousarray(table, np.int32)
    assert table.size >= info.n_ref + info.n_sig + info.n_sign
    _check(load().picsong_lut_save(os.fsencode(folder), component, C.byref(info), wl, table.ctypes.data_as(C.c_void_p)))


def make_params(width, height, wl=5, lossy=False, qs=1.0, frames=0, rgb=False, k=0.0, cp=2, bit_depth=8):
    return Params(width=width, height=height, wl=wl, cp=cp, lossy=int(lossy), qs=qs, k=k,
                  cb_width=64, cb_height=18, bit_depth=bit_depth, frames=frames, components=3 if rgb else 1,
                  is_rgb=int(rgb))


def depth_range_guaranteed(bit_depth, lossy, wl, qs=1.0):
    """Does every frame of `bit_depth`-bit samples keep its coefficients below the coders' 2^15
    (picsong_depth_range_guaranteed)?  Where not, a frame that reaches it raises the range flag."""
    yes = C.c_int()
    _check(load().picsong_depth_range_guaranteed(bit_depth, int(lossy), wl, qs, C.byref(yes)))
    return bool(yes.value)


def depth_range_guaranteed_rgb(bit_depth, lossy, wl, qs=1.0):
    """The same question for a deep RGB context (picsong_depth_range_guaranteed_rgb): the RCT's chroma components span one
    bit more than a grey sample, the ICT's components as much as one."""
    yes = C.c_int()
    _check(load().picsong_depth_range_guaranteed_rgb(bit_depth, int(lossy), wl, qs, C.byref(yes)))
    return bool(yes.value)


def pad_frame16(img_u16, aw, ah):
    """picsong_pad_frame16_host: the (H, W) uint16 frame mirror-padded to (ah, aw)."""
    img_u16 = np.ascontiguousarray(img_u16, np.uint16)
    h, w = img_u16.shape
    out = np.zeros((ah, aw), np.uint16)
    _check(load().picsong_pad_frame16_host(img_u16.ctypes.data_as(C.c_void_p), w, h, out.ctypes.data_as(C.c_void_p), aw, ah))
    return out


def header_pack(params):
    out = np.zeros(9, np.uint16)
    _check(load().picsong_header_pack(C.byref(params), out.ctypes.data_as(C.c_void_p)))
    return out


def header_unpack(shorts):
    shorts = np.ascontiguousarray(shorts, np.uint16)
    p = Params()
    _check(load().picsong_header_unpack(shorts.ctypes.data_as(C.c_void_p), C.byref(p)))
    return p


class Codec:
    """One coding context (== the reference's per-frame DWT<T,Y> / BPCCuda<T> / BitStreamBuilder
    objects + the LUT upload of Engine::initLUT).  All tensor arguments are torch CUDA tensors."""

    def __init__(self, width, height, wl=5, lossy=False, qs=1.0, lut_folder=None, lut_fill=0,
                 device=0, frames=0, rgb=False, k=0.0, pipelined=False, cp=2, bit_depth=8, is_rgb=False):
        """rgb: an 8-bit RGB context, whose methods take and return uint8 planes (encode_rgb_frame and its kin) -- with
        bit_depth 9..16 it is refused here, as it always was.  is_rgb (with bit_depth 9..16): a deep RGB context, three uint16
        planes a frame through the *16 RGB methods; with bit_depth 8 it is rgb."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the picsong HIP path has no CPU fallback")
        self.torch = torch
        self.L = load()
        if rgb and bit_depth != 8:
            raise PicsongError(f"Codec(rgb=True) is the 8-bit RGB context (uint8 planes); {bit_depth}-bit colour: Codec(bit_depth={bit_depth}, "
                               "is_rgb=True), uint16 planes through encode_rgb_frames16 / decode_rgb_frames16")
        rgb = bool(rgb or is_rgb)
        self.params = make_params(width, height, wl, lossy, qs, frames, rgb, k, cp, bit_depth)
        self.bit_depth = bit_depth
        self.rgb = rgb
        self.device = device
        h = C.c_void_p()
        _check(self.L.picsong_ctx_create(C.byref(self.params), device, C.byref(h)))
        self.h = h
        if pipelined:                 # frames of other contexts share the GPU: throughput over latency
            _check(self.L.picsong_ctx_set_pipelined(self.h, 1))
        aw, ah, ncb = C.c_int(), C.c_int(), C.c_int()
        _check(self.L.picsong_ctx_padded_dims(self.h, C.byref(aw), C.byref(ah), C.byref(ncb)))
        self.aw, self.ah, self.ncb = aw.value, ah.value, ncb.value
        self.P = self.aw * self.ah
        self.extra = dwt_extra(self.aw, self.ah, wl)
        self.lossy = bool(lossy)
        self.dtype = torch.float32 if lossy else torch.int32
        self.dev = torch.device("cuda", device)
        if lut_folder is not None:
            for comp in range(3 if rgb else 1):
                # files ...R/G/B.txt_0 (k = 0) or every bit-plane file ...txt_0.._14 (k > 0)
                info, table = lut_load(lut_folder, wl, comp + 1, lut_fill, 0 if k > 0 else 1, cp)
                self.set_lut(info, table, comp)

    def close(self):
        if getattr(self, "h", None):
            self.L.picsong_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    @staticmethod
    def _p(t):
        return C.c_void_p(t.data_ptr())

    def set_lut(self, info, table, component=0):
        table = np.ascontiguousarray(table, np.int32)
        _check(self.L.picsong_ctx_set_lut_component(self.h, component, C.byref(info),
                                                    table.ctypes.data_as(C.c_void_p)))

    def set_decode_drop(self, drop):
        """Decode at reduced quality from now on: a codeblock of level lv leaves its max(0, drop - lv) lowest bit-planes
        undecoded, significant coefficients get the midpoint (picsong_ctx_set_decode_drop).  0..15, 0 = the plain
        decode; k = 0, -cp 2 contexts.  Every decode call of the context follows it; encodes and searches do not."""
        _check(self.L.picsong_ctx_set_decode_drop(self.h, int(drop)))

    def decode_drop(self):
        d = C.c_int()
        _check(self.L.picsong_ctx_get_decode_drop(self.h, C.byref(d)))
        return d.value

    # ---- frames as applications hold them: pitched, unpadded, interleaved RGB(A) (picsong_image) ----
    def image(self, t, layout, pitch=None, plane_stride=0, offset=0):
        """The picsong_image of the uint8 CUDA tensor `t` (any shape; its storage from byte `offset` on is the frame):
        rows `pitch` bytes apart (default: packed, W * bpp), PLANAR3 planes plane_stride bytes apart."""
        assert (t.dtype == self.torch.uint8 or layout in LAYOUTS_16) and t.is_cuda
        pitch = self.params.width * LAYOUT_BPP[layout] if pitch is None else pitch
        return Image(data=t.data_ptr() + offset, pitch=pitch, plane_stride=plane_stride, layout=layout)

    def ingest_frames(self, img, n=1, frame_stride=0, out=None):
        """n frames of `img` (an Image; frame f frame_stride bytes behind frame 0) to padded planar planes on the device:
        uint8 [n, planes, AH, AW] (planes: 1 for GREY8, else R, G, B), mirror-padded as picsong_pad_frame_host pads."""
        planes = 1 if img.layout in (LAYOUT_GREY8, LAYOUT_GREY16) else 3
        if out is None:                                  # (the 16-bit layouts: int16 tensors holding the uint16 samples)
            out = self.torch.empty((n, planes, self.ah, self.aw), dtype=self.torch.int16 if img.layout in LAYOUTS_16 else self.torch.uint8,
                                   device=self.dev)
        _check(self.L.picsong_ingest_frames(self.h, n, C.byref(img), frame_stride, self._p(out), out.stride(0) * out.element_size(),
                                            self._stream()))
        return out

    def emit_frames(self, padded, img, n=1, frame_stride=0):
        """The inverse: uint8 [n, planes, AH, AW] padded planes cropped and interleaved into the frames of `img`."""
        assert padded.stride(-1) == 1
        _check(self.L.picsong_emit_frames(self.h, n, self._p(padded), padded.stride(0) * padded.element_size() if padded.dim() == 4 else 0, C.byref(img),
                                          frame_stride, self._stream()))

    def encode_images(self, img, n=1, frame_stride=0, first_iter=0):
        """n grey frames of `img` ingested on the device and coded as encode_frames codes host-padded ones."""
        out = self.torch.empty((n, self.max_stream_shorts()), dtype=self.torch.int16, device=self.dev)
        _check(self.L.picsong_encode_images(self.h, n, C.byref(img), frame_stride, first_iter, self._p(out), out.stride(0),
                                            self._stream()))
        return [out[k, :t] for k, t in enumerate(self.last_totals(n))]

    def decode_images(self, streams, img, frame_stride=0):
        """streams: int16 [n, >= max_stream_shorts()]; the W x H frames land in `img` (frame f frame_stride bytes on)."""
        assert streams.stride(-1) == 1
        _check(self.L.picsong_decode_images(self.h, streams.shape[0], self._p(streams), streams.stride(0), C.byref(img), frame_stride,
                                            self._stream()))

    def encode_rgb_image(self, img, header_mask=1):
        """One RGB frame of `img` (any colour layout) as encode_rgb_frame codes its host-padded planes."""
        out = self.torch.empty((3, self.max_stream_shorts()), dtype=self.torch.int16, device=self.dev)
        _check(self.L.picsong_encode_rgb_image(self.h, C.byref(img), header_mask, self._p(out), out.stride(0), self._stream()))
        totals = self.last_totals(3)
        return [out[k, :totals[k]] for k in range(3)]

    def decode_rgb_image(self, streams, img):
        """streams: int16 [3, >= max_stream_shorts()]; the W x H pixels land in `img`, alpha (if any) 255."""
        _check(self.L.picsong_decode_rgb_image(self.h, self._p(streams), streams.stride(0), C.byref(img), self._stream()))

    # ---- rate control: the 9/7 encode calls with qs chosen to meet a size (synchronous) ----
    def set_qs(self, qs):
        """The context's qs from now on (picsong_ctx_set_qs): tables and buffers stay."""
        _check(self.L.picsong_ctx_set_qs(self.h, qs))
        self.params.qs = qs

    def encode_frame_rate(self, frame_u8_padded, target_shorts, j_min=0, j_max=0, iter_=0, out=None):
        """Returns (j, codestream): the stream of picsong_encode_frame at qs = rate_qs(j), j the quantiser search's
        result for target_shorts; raises RateError when nothing of the range fits."""
        if out is None:
            out = self.torch.empty(self.max_stream_shorts(), dtype=self.torch.int16, device=self.dev)
        j, t = C.c_int(), C.c_int()
        _check_rate(self.L.picsong_encode_frame_rate(self.h, self._p(frame_u8_padded), iter_, target_shorts, j_min, j_max,
                                                     self._p(out), self._stream(), C.byref(j), C.byref(t)))
        return j.value, out[:t.value]

    def encode_frames_rate(self, frames_u8_padded, target_shorts, j_min=0, j_max=0, first_iter=0):
        """frames_u8_padded: uint8 [n, AH*AW], n <= 16; target_shorts for the sum of the n streams.  Returns (j, streams)."""
        n = frames_u8_padded.shape[0]
        assert frames_u8_padded.stride(-1) == 1
        out = self.torch.empty((n, self.max_stream_shorts()), dtype=self.torch.int16, device=self.dev)
        j, t = C.c_int(), (C.c_int * n)()
        _check_rate(self.L.picsong_encode_frames_rate(self.h, n, self._p(frames_u8_padded), frames_u8_padded.stride(0),
                                                      first_iter, target_shorts, j_min, j_max, self._p(out), out.stride(0),
                                                      self._stream(), C.byref(j), t))
        return j.value, [out[f, :t[f]] for f in range(n)]

    def encode_rgb_frame_rate(self, r, g, b, target_shorts, j_min=0, j_max=0, header_mask=1):
        """target_shorts for the sum of the three components' streams.  Returns (j, the three codestreams)."""
        out = self.torch.empty((3, self.max_stream_shorts()), dtype=self.torch.int16, device=self.dev)
        j, t = C.c_int(), (C.c_int * 3)()
        _check_rate(self.L.picsong_encode_rgb_frame_rate(self.h, self._p(r), self._p(g), self._p(b), header_mask,
                                                         target_shorts, j_min, j_max, self._p(out), out.stride(0),
                                                         self._stream(), C.byref(j), t))
        return j.value, [out[k, :t[k]] for k in range(3)]

    # ---- quality control: distortion measurement, and the 9/7 encode calls with qs chosen to meet an SSE limit ----
    def frames_sse(self, a, b, out=None):
        """a, b: uint8 padded frames [n, AH*AW] (or one frame [AH*AW]); returns an int64 device tensor [n] holding the SSE
        over the visible samples of each pair (picsong_frames_sse, asynchronous)."""
        if a.dim() == 1:
            a, b = a[None], b[None]
        n = a.shape[0]
        assert b.shape[0] == n and a.stride(-1) == 1 and b.stride(-1) == 1
        if out is None:
            out = self.torch.empty(n, dtype=self.torch.int64, device=self.dev)
        _check(self.L.picsong_frames_sse(self.h, n, self._p(a), a.stride(0), self._p(b), b.stride(0), self._p(out),
                                         self._stream()))
        return out

    def encode_frame_quality(self, frame_u8_padded, max_sse, j_min=0, j_max=0, iter_=0, out=None):
        """Returns (j, codestream, sse): the stream of picsong_encode_frame at qs = rate_qs(j), j the quantiser search's
        result for max_sse; raises QualityError when nothing of the range meets it."""
        if out is None:
            out = self.torch.empty(self.max_stream_shorts(), dtype=self.torch.int16, device=self.dev)
        j, t, e = C.c_int(), C.c_int(), C.c_uint64()
        _check_quality(self.L.picsong_encode_frame_quality(self.h, self._p(frame_u8_padded), iter_, max_sse, j_min, j_max,
                                                           self._p(out), self._stream(), C.byref(j), C.byref(t), C.byref(e)))
        return j.value, out[:t.value], e.value

    def encode_frames_quality(self, frames_u8_padded, max_sse, j_min=0, j_max=0, first_iter=0):
        """frames_u8_padded: uint8 [n, AH*AW], n <= 16; max_sse for the sum over the n frames.  Returns (j, streams, the
        per-frame SSE)."""
        n = frames_u8_padded.shape[0]
        assert frames_u8_padded.stride(-1) == 1
        out = self.torch.empty((n, self.max_stream_shorts()), dtype=self.torch.int16, device=self.dev)
        j, t, e = C.c_int(), (C.c_int * n)(), (C.c_uint64 * n)()
        _check_quality(self.L.picsong_encode_frames_quality(self.h, n, self._p(frames_u8_padded), frames_u8_padded.stride(0),
                                                            first_iter, max_sse, j_min, j_max, self._p(out), out.stride(0),
                                                            self._stream(), C.byref(j), t, e))
        return j.value, [out[f, :t[f]] for f in range(n)], [int(v) for v in e]

    def encode_rgb_frame_quality(self, r, g, b, max_sse, j_min=0, j_max=0, header_mask=1):
        """max_sse for the sum over the three planes.  Returns (j, the three codestreams, the SSE of R, G, B)."""
        out = self.torch.empty((3, self.max_stream_shorts()), dtype=self.torch.int16, device=self.dev)
        j, t, e = C.c_int(), (C.c_int * 3)(), (C.c_uint64 * 3)()
        _check_quality(self.L.picsong_encode_rgb_frame_quality(self.h, self._p(r), self._p(g), self._p(b), header_mask,
                                                               max_sse, j_min, j_max, self._p(out), out.stride(0),
                                                               self._stream(), C.byref(j), t, e))
        return j.value, [out[k, :t[k]] for k in range(3)], [int(v) for v in e]

    # ---- SSIM control: the structural measure, and the 9/7 encode calls with qs chosen to meet a DSSIM-sum limit ----
    def frames_dssim(self, a, b, out=None):
        """a, b: uint8 padded frames [n, AH*AW] (or one frame [AH*AW]); returns an int64 device tensor [n] holding the
        DSSIM sum over the visible samples of each pair (picsong_frames_dssim, asynchronous)."""
        if a.dim() == 1:
            a, b = a[None], b[None]
        n = a.shape[0]
        assert b.shape[0] == n and a.stride(-1) == 1 and b.stride(-1) == 1
        if out is None:
            out = self.torch.empty(n, dtype=self.torch.int64, device=self.dev)
        _check(self.L.picsong_frames_dssim(self.h, n, self._p(a), a.stride(0), self._p(b), b.stride(0), self._p(out),
                                           self._stream()))
        return out

    def encode_frame_ssim(self, frame_u8_padded, max_dssim, j_min=0, j_max=0, iter_=0, out=None):
        """Returns (j, codestream, dssim): the stream of picsong_encode_frame at qs = rate_qs(j), j the quantiser search's
        result for max_dssim; raises QualityError when nothing of the range meets it."""
        if out is None:
            out = self.torch.empty(self.max_stream_shorts(), dtype=self.torch.int16, device=self.dev)
        j, t, e = C.c_int(), C.c_int(), C.c_uint64()
        _check_quality(self.L.picsong_encode_frame_ssim(self.h, self._p(frame_u8_padded), iter_, max_dssim, j_min, j_max,
                                                        self._p(out), self._stream(), C.byref(j), C.byref(t), C.byref(e)))
        return j.value, out[:t.value], e.value

    def encode_frames_ssim(self, frames_u8_padded, max_dssim, j_min=0, j_max=0, first_iter=0):
        """frames_u8_padded: uint8 [n, AH*AW], n <= 16; max_dssim for the sum over the n frames.  Returns (j, streams, the
        per-frame DSSIM sums)."""
        n = frames_u8_padded.shape[0]
        assert frames_u8_padded.stride(-1) == 1
        out = self.torch.empty((n, self.max_stream_shorts()), dtype=self.torch.int16, device=self.dev)
        j, t, e = C.c_int(), (C.c_int * n)(), (C.c_uint64 * n)()
        _check_quality(self.L.picsong_encode_frames_ssim(self.h, n, self._p(frames_u8_padded), frames_u8_padded.stride(0),
                                                         first_iter, max_dssim, j_min, j_max, self._p(out), out.stride(0),
                                                         self._stream(), C.byref(j), t, e))
        return j.value, [out[f, :t[f]] for f in range(n)], [int(v) for v in e]

    def encode_rgb_frames_ssim(self, r, g, b, max_dssim, j_min=0, j_max=0, n=None, frame_stride=None, first_iter=0,
                               header_mask=7):
        """max_dssim for the sum over the 3 n planes (r / g / b as encode_rgb_frames takes them).  Returns (j, the 3 n
        codestreams, the DSSIM sum per plane: frame f's R, G, B at 3 f ..)."""
        n, frame_stride = self._rgb_frames_span(r, g, b, n, frame_stride)
        out = self.torch.empty((3 * n, self.max_stream_shorts()), dtype=self.torch.int16, device=self.dev)
        j, t, e = C.c_int(), (C.c_int * (3 * n))(), (C.c_uint64 * (3 * n))()
        _check_quality(self.L.picsong_encode_rgb_frames_ssim(self.h, n, self._p(r), self._p(g), self._p(b), frame_stride,
                                                             first_iter, header_mask, max_dssim, j_min, j_max, self._p(out),
                                                             out.stride(0), self._stream(), C.byref(j), t, e))
        return j.value, [out[k, :t[k]] for k in range(3 * n)], [int(v) for v in e]

    # ---- training: the statistics a probability table is made from (k = 0, -cp 2 contexts; no table needed) ----
    def train_begin(self, **geometry):
        """Allocate and zero the counters; geometry fields default to the shipped folders' (TRAIN_GEOMETRY)."""
        info = LutInfo(**dict(TRAIN_GEOMETRY, **geometry))
        _check(self.L.picsong_train_begin(self.h, C.byref(info)))
        return self.train_info()

    def train_info(self):
        info = LutInfo()
        _check(self.L.picsong_train_info(self.h, C.byref(info)))
        return info

    def train_reset(self):
        _check(self.L.picsong_train_reset(self.h))

    def train_end(self):
        _check(self.L.picsong_train_end(self.h))

    def train_coeffs(self, coef, component=0):
        """coef: the Mallat array as bpc_encode takes it (int32 / float32 device tensor of AW*AH elements)."""
        _check(self.L.picsong_train_coeffs(self.h, component, self._p(coef), self._stream()))

    def train_frames(self, frames_u8_padded):
        """frames_u8_padded: uint8 [n, AH*AW] (or [n, AH, AW]) device tensor, rows contiguous; into slot 0."""
        n = frames_u8_padded.shape[0]
        assert frames_u8_padded.stride(-1) == 1
        _check(self.L.picsong_train_frames(self.h, n, self._p(frames_u8_padded), frames_u8_padded.stride(0), self._stream()))

    def train_rgb_frame(self, r, g, b):
        _check(self.L.picsong_train_rgb_frame(self.h, self._p(r), self._p(g), self._p(b), self._stream()))

    def train_counts(self, component=0):
        """uint64 [entries, 2] (zeros, ones) of a component slot; synchronises."""
        n = self.L.picsong_train_counts(self.h, component, self._stream(), None, 0)
        if n < 0:
            _check(n)
        out = np.zeros((n, 2), np.uint64)
        _check(self.L.picsong_train_counts(self.h, component, self._stream(), out.ctypes.data_as(C.c_void_p), n))
        return out

    # ---- RGB path ----
    def rgb_forward(self, r, g, b):
        outs = [self.torch.empty(self.P, dtype=self.dtype, device=self.dev) for _ in range(3)]
        _check(self.L.picsong_rgb_forward(self.h, self._p(r), self._p(g), self._p(b), self._p(outs[0]),
                                          self._p(outs[1]), self._p(outs[2]), self._stream()))
        return outs

    def rgb_inverse(self, c0, c1, c2):
        outs = [self.torch.empty(self.P, dtype=self.torch.uint8, device=self.dev) for _ in range(3)]
        _check(self.L.picsong_rgb_inverse(self.h, self._p(c0), self._p(c1), self._p(c2), self._p(outs[0]),
                                          self._p(outs[1]), self._p(outs[2]), self._stream()))
        return [o.view(self.ah, self.aw) for o in outs]

    def encode_plane(self, plane, component, with_header):
        out = self.torch.empty(self.max_stream_shorts(), dtype=self.torch.int16, device=self.dev)
        _check(self.L.picsong_encode_plane(self.h, self._p(plane), component, int(with_header), self._p(out),
                                           self._stream()))
        return out[:self.last_total()]

    def encode_rgb_frame(self, r, g, b, header_mask=1):
        """One RGB frame (padded u8 planes) through one launch per stage; returns the three codestreams."""
        out = self.torch.empty((3, self.max_stream_shorts()), dtype=self.torch.int16, device=self.dev)
        _check(self.L.picsong_encode_rgb_frame(self.h, self._p(r), self._p(g), self._p(b), header_mask, self._p(out),
                                               out.stride(0), self._stream()))
        totals = self.last_totals(3)
        return [out[k, :totals[k]] for k in range(3)]

    def decode_rgb_frame(self, streams):
        """streams: int16 [3, >= max_stream_shorts()]; returns the three padded u8 planes."""
        outs = [self.torch.empty((self.ah, self.aw), dtype=self.torch.uint8, device=self.dev) for _ in range(3)]
        _check(self.L.picsong_decode_rgb_frame(self.h, self._p(streams), streams.stride(0), self._p(outs[0]),
                                               self._p(outs[1]), self._p(outs[2]), self._stream()))
        return outs

    # ---- batched RGB frames: n colour frames through one launch per stage, 3 n planes a launch ----
    def encode_rgb_frames(self, r, g, b, n=None, frame_stride=None, first_iter=0, header_mask=7):
        """n RGB frames; r / g / b: uint8 [n, AH, AW] tensors (frame f at stride(0) bytes behind frame 0, the same for all
        three), or frame 0's planes with n and frame_stride given.  Returns the 3 n codestreams, frame f's component c at
        index 3 f + c; the populated header on the components of header_mask of the frame with first_iter + f == 0."""
        if n is None:
            n = r.shape[0]
        if frame_stride is None:
            frame_stride = r.stride(0) if n > 1 else 0
            assert n == 1 or (g.stride(0) == frame_stride and b.stride(0) == frame_stride)
        out = self.torch.empty((3 * n, self.max_stream_shorts()), dtype=self.torch.int16, device=self.dev)
        _check(self.L.picsong_encode_rgb_frames(self.h, n, self._p(r), self._p(g), self._p(b), frame_stride, first_iter, header_mask,
                                                self._p(out), out.stride(0), self._stream()))
        return [out[k, :t] for k, t in enumerate(self.last_totals(3 * n))]

    def _rgb_frames_span(self, r, g, b, n, frame_stride):
        if n is None:
            n = r.shape[0]
        if frame_stride is None:
            frame_stride = r.stride(0) if n > 1 else 0
            assert n == 1 or (g.stride(0) == frame_stride and b.stride(0) == frame_stride)
        return n, frame_stride

    def encode_rgb_frames_rate(self, r, g, b, target_shorts, j_min=0, j_max=0, n=None, frame_stride=None, first_iter=0,
                               header_mask=7):
        """The quantiser search over n RGB frames (r / g / b as encode_rgb_frames takes them); target_shorts for the sum
        of the 3 n streams.  Returns (j, the 3 n codestreams, frame f's component c at index 3 f + c)."""
        n, frame_stride = self._rgb_frames_span(r, g, b, n, frame_stride)
        out = self.torch.empty((3 * n, self.max_stream_shorts()), dtype=self.torch.int16, device=self.dev)
        j, t = C.c_int(), (C.c_int * (3 * n))()
        _check_rate(self.L.picsong_encode_rgb_frames_rate(self.h, n, self._p(r), self._p(g), self._p(b), frame_stride, first_iter,
                                                          header_mask, target_shorts, j_min, j_max, self._p(out), out.stride(0),
                                                          self._stream(), C.byref(j), t))
        return j.value, [out[k, :t[k]] for k in range(3 * n)]

    def encode_rgb_frames_quality(self, r, g, b, max_sse, j_min=0, j_max=0, n=None, frame_stride=None, first_iter=0,
                                  header_mask=7):
        """max_sse for the sum over the 3 n planes.  Returns (j, the 3 n codestreams, the SSE per plane: frame f's R, G, B
        at 3 f ..)."""
        n, frame_stride = self._rgb_frames_span(r, g, b, n, frame_stride)
        out = self.torch.empty((3 * n, self.max_stream_shorts()), dtype=self.torch.int16, device=self.dev)
        j, t, e = C.c_int(), (C.c_int * (3 * n))(), (C.c_uint64 * (3 * n))()
        _check_quality(self.L.picsong_encode_rgb_frames_quality(self.h, n, self._p(r), self._p(g), self._p(b), frame_stride,
                                                                first_iter, header_mask, max_sse, j_min, j_max, self._p(out),
                                                                out.stride(0), self._stream(), C.byref(j), t, e))
        return j.value, [out[k, :t[k]] for k in range(3 * n)], [int(v) for v in e]

    def train_rgb_frames(self, r, g, b, n=None, frame_stride=None):
        """n RGB frames' statistics, component c of every frame into slot c (picsong_train_rgb_frames)."""
        n, frame_stride = self._rgb_frames_span(r, g, b, n, frame_stride)
        _check(self.L.picsong_train_rgb_frames(self.h, n, self._p(r), self._p(g), self._p(b), frame_stride, self._stream()))

    def decode_rgb_frames(self, streams, outs=None, frame_stride=None):
        """streams: int16 [3 n, >= max_stream_shorts()]; returns the R, G, B planes as three uint8 [n, AH, AW] tensors
        (or writes frame f's planes frame_stride bytes behind outs[0..2], frame 0's)."""
        assert streams.stride(-1) == 1 and streams.shape[0] % 3 == 0
        n = streams.shape[0] // 3
        if outs is None:
            outs = [self.torch.empty((n, self.ah, self.aw), dtype=self.torch.uint8, device=self.dev) for _ in range(3)]
            frame_stride = outs[0].stride(0)
        _check(self.L.picsong_decode_rgb_frames(self.h, n, self._p(streams), streams.stride(0), self._p(outs[0]), self._p(outs[1]),
                                                self._p(outs[2]), frame_stride or 0, self._stream()))
        return outs

    def encode_rgb_images(self, img, n=1, frame_stride=0, first_iter=0, header_mask=7):
        """n RGB frames of `img` (any colour layout; frame f frame_stride bytes behind frame 0), ingested on the device in
        one launch and coded as encode_rgb_frames codes their host-padded planes."""
        out = self.torch.empty((3 * n, self.max_stream_shorts()), dtype=self.torch.int16, device=self.dev)
        _check(self.L.picsong_encode_rgb_images(self.h, n, C.byref(img), frame_stride, first_iter, header_mask, self._p(out),
                                                out.stride(0), self._stream()))
        return [out[k, :t] for k, t in enumerate(self.last_totals(3 * n))]

    def decode_rgb_images(self, streams, img, frame_stride=0):
        """streams: int16 [3 n, >= max_stream_shorts()]; the n W x H frames land in `img`, alpha (if any) 255."""
        assert streams.stride(-1) == 1 and streams.shape[0] % 3 == 0
        _check(self.L.picsong_decode_rgb_images(self.h, streams.shape[0] // 3, self._p(streams), streams.stride(0), C.byref(img),
                                                frame_stride, self._stream()))

    def decode_plane(self, stream, component):
        out = self.torch.empty(self.P + self.extra, dtype=self.dtype, device=self.dev)
        _check(self.L.picsong_decode_plane(self.h, self._p(stream), component, self._p(out), self._stream()))
        return out[self.extra:]

    # ---- stage functions (device tensors in/out) ----
    def level_shift_fwd(self, u8):
        out = self.torch.empty(self.P, dtype=self.dtype, device=self.dev)
        _check(self.L.picsong_level_shift_fwd(self.h, self._p(u8), self._p(out), self._stream()))
        return out

    def level_shift_inv(self, data):
        _check(self.L.picsong_level_shift_inv(self.h, self._p(data), self._stream()))
        return data

    def dwt_forward(self, x):
        out = self.torch.zeros(self.P + self.extra, dtype=self.dtype, device=self.dev)
        fn = self.L.picsong_dwt_forward_u8 if x.dtype == self.torch.uint8 else self.L.picsong_dwt_forward
        _check(fn(self.h, self._p(x), self._p(out), self._stream()))
        return out

    def dwt_inverse(self, coef_i32):
        out = self.torch.zeros(self.P + self.extra, dtype=self.dtype, device=self.dev)
        _check(self.L.picsong_dwt_inverse(self.h, self._p(coef_i32), self._p(out), self._stream()))
        return out

    def bpc_encode(self, coef):
        staging = self.torch.empty(self.P, dtype=self.torch.int32, device=self.dev)
        sizes = self.torch.empty(self.ncb, dtype=self.torch.int32, device=self.dev)
        _check(self.L.picsong_bpc_encode(self.h, self._p(coef), self._p(staging), self._p(sizes),
                                         self._stream()))
        return staging, sizes

    def bpc_decode(self, staging, sizes):
        coef = self.torch.empty(self.P, dtype=self.torch.int32, device=self.dev)
        _check(self.L.picsong_bpc_decode(self.h, self._p(staging), self._p(sizes), self._p(coef),
                                         self._stream()))
        return coef

    def bitstream_pack(self, staging, sizes, header=None):
        out = self.torch.empty(self.max_stream_shorts(), dtype=self.torch.int16, device=self.dev)
        total = C.c_int()
        hp = None
        if header is not None:
            header = np.ascontiguousarray(header, np.uint16)
            hp = header.ctypes.data_as(C.c_void_p)
        _check(self.L.picsong_bitstream_pack(self.h, self._p(staging), self._p(sizes), hp, self._p(out),
                                             C.byref(total), self._stream()))
        return out[:total.value]

    def bitstream_unpack(self, stream):
        staging = self.torch.empty(self.P, dtype=self.torch.int32, device=self.dev)
        sizes = self.torch.empty(self.ncb, dtype=self.torch.int32, device=self.dev)
        _check(self.L.picsong_bitstream_unpack(self.h, self._p(stream), self._p(staging), self._p(sizes),
                                               self._stream()))
        return staging, sizes

    def max_stream_shorts(self):
        return self.L.picsong_max_stream_shorts(self.aw, self.ah)

    def range_flag(self):
        f = C.c_int()
        _check(self.L.picsong_range_flag(self.h, self._stream(), C.byref(f)))
        return f.value

    def profile_begin(self, capacity):
        _check(self.L.picsong_profile_begin(self.h, capacity))

    def profile_read(self, capacity):
        """(n, 3) float32 array of {dwt_ms, bpc_ms, pack_ms} per encode_frame since profile_begin."""
        ms = np.zeros((capacity, 3), np.float32)
        n = C.c_int()
        _check(self.L.picsong_profile_read(self.h, C.byref(n), ms.ctypes.data_as(C.c_void_p), capacity))
        return ms[:n.value]

    # ---- deep contexts (bit_depth 9..16): uint16 samples, held in int16 tensors (torch's 16-bit integer type; the bits
    # are the unsigned samples': numpy's .view(np.uint16) on the host) ----
    def level_shift_fwd16(self, u16):
        out = self.torch.empty(self.P, dtype=self.dtype, device=self.dev)
        _check(self.L.picsong_level_shift_fwd16(self.h, self._p(u16), self._p(out), self._stream()))
        return out

    def dwt_forward_u16(self, u16):
        out = self.torch.zeros(self.P + self.extra, dtype=self.dtype, device=self.dev)
        _check(self.L.picsong_dwt_forward_u16(self.h, self._p(u16), self._p(out), self._stream()))
        return out

    def encode_frames16(self, frames_u16_padded, first_iter=0, frame_stride=None):
        """frames_u16_padded: int16 [n, AH*AW] or [n, AH, AW] (frame f stride(0) elements behind frame 0, or frame_stride
        BYTES where given); returns the n codestreams."""
        n = frames_u16_padded.shape[0]
        assert frames_u16_padded.element_size() == 2 and frames_u16_padded.stride(-1) == 1
        if frame_stride is None:
            frame_stride = 2 * frames_u16_padded.stride(0)
        out = self.torch.empty((n, self.max_stream_shorts()), dtype=self.torch.int16, device=self.dev)
        _check(self.L.picsong_encode_frames16(self.h, n, self._p(frames_u16_padded), frame_stride, first_iter, self._p(out),
                                              out.stride(0), self._stream()))
        return [out[k, :t] for k, t in enumerate(self.last_totals(n))]

    def decode_frames16(self, streams, out=None, frame_stride=None):
        """streams: int16 [n, >= max_stream_shorts()]; returns int16 [n, AH, AW] holding the uint16 samples (or writes frame
        f frame_stride BYTES behind `out`)."""
        n = streams.shape[0]
        assert streams.stride(-1) == 1
        if out is None:
            out = self.torch.empty((n, self.ah, self.aw), dtype=self.torch.int16, device=self.dev)
        if frame_stride is None:
            frame_stride = 2 * out.stride(0)
        _check(self.L.picsong_decode_frames16(self.h, n, self._p(streams), streams.stride(0), self._p(out), frame_stride,
                                              self._stream()))
        return out

    # ---- deep RGB contexts (Codec(bit_depth=9..16, is_rgb=True)): three uint16 planes a frame, int16 tensors as above ----
    def rgb_forward16(self, r, g, b):
        outs = [self.torch.empty(self.P, dtype=self.dtype, device=self.dev) for _ in range(3)]
        _check(self.L.picsong_rgb_forward16(self.h, self._p(r), self._p(g), self._p(b), self._p(outs[0]), self._p(outs[1]),
                                            self._p(outs[2]), self._stream()))
        return outs

    def rgb_inverse16(self, c0, c1, c2):
        outs = [self.torch.empty((self.ah, self.aw), dtype=self.torch.int16, device=self.dev) for _ in range(3)]
        _check(self.L.picsong_rgb_inverse16(self.h, self._p(c0), self._p(c1), self._p(c2), self._p(outs[0]), self._p(outs[1]),
                                            self._p(outs[2]), self._stream()))
        return outs

    def encode_rgb_frames16(self, r, g, b, n=None, frame_stride=None, first_iter=0, header_mask=7):
        """n deep RGB frames; r / g / b: int16 [n, AH, AW] tensors (frame f stride(0) elements behind frame 0, the same for
        all three), or frame 0's planes with n and frame_stride (BYTES) given.  Returns the 3 n codestreams, frame f's
        component c at index 3 f + c."""
        if n is None:
            n = r.shape[0]
        if frame_stride is None:
            frame_stride = 2 * r.stride(0) if n > 1 else 0
            assert n == 1 or (g.stride(0) == r.stride(0) and b.stride(0) == r.stride(0))
        out = self.torch.empty((3 * n, self.max_stream_shorts()), dtype=self.torch.int16, device=self.dev)
        _check(self.L.picsong_encode_rgb_frames16(self.h, n, self._p(r), self._p(g), self._p(b), frame_stride, first_iter, header_mask,
                                                  self._p(out), out.stride(0), self._stream()))
        return [out[k, :t] for k, t in enumerate(self.last_totals(3 * n))]

    def decode_rgb_frames16(self, streams, outs=None, frame_stride=None):
        """streams: int16 [3 n, >= max_stream_shorts()]; returns the R, G, B planes as three int16 [n, AH, AW] tensors holding
        the uint16 samples (or writes frame f's planes frame_stride BYTES behind outs[0..2], frame 0's)."""
        assert streams.stride(-1) == 1 and streams.shape[0] % 3 == 0
        n = streams.shape[0] // 3
        if outs is None:
            outs = [self.torch.empty((n, self.ah, self.aw), dtype=self.torch.int16, device=self.dev) for _ in range(3)]
            frame_stride = 2 * outs[0].stride(0)
        _check(self.L.picsong_decode_rgb_frames16(self.h, n, self._p(streams), streams.stride(0), self._p(outs[0]), self._p(outs[1]),
                                                  self._p(outs[2]), frame_stride or 0, self._stream()))
        return outs

    # ---- deep proxies: deep frames at 1/2^r, or a window of them; uint16 samples in int16 tensors, strides in bytes ----
    def decode_frames16_reduced(self, streams, r, out=None, frame_stride=None):
        """streams: int16 [n, >= max_stream_shorts()]; returns int16 [n, AH >> r, AW >> r] holding the uint16 samples (or
        writes frame f frame_stride BYTES behind `out`)."""
        n = streams.shape[0]
        assert streams.stride(-1) == 1
        if out is None:
            out = self.torch.empty((n, self.ah >> r, self.aw >> r), dtype=self.torch.int16, device=self.dev)
        if frame_stride is None:
            frame_stride = 2 * out.stride(0)
        _check(self.L.picsong_decode_frames16_reduced(self.h, n, self._p(streams), streams.stride(0), r, self._p(out), frame_stride,
                                                      self._stream()))
        return out

    def decode_frames16_window(self, streams, x, y, w, h, r=0, out=None):
        """streams: int16 [n, >= max_stream_shorts()]; returns int16 [n, h, w] (or fills `out`, a 3-D int16 view: frame
        stride out.stride(0), pitch out.stride(1), in elements)."""
        n = streams.shape[0]
        assert streams.stride(-1) == 1
        if out is None:
            out = self.torch.empty((n, h, w), dtype=self.torch.int16, device=self.dev)
        assert out.dtype == self.torch.int16 and tuple(out.shape) == (n, h, w) and out.stride(2) == 1
        _check(self.L.picsong_decode_frames16_window(self.h, n, self._p(streams), streams.stride(0), r, x, y, w, h, self._p(out),
                                                     2 * out.stride(1), 2 * out.stride(0), self._stream()))
        return out

    def decode_rgb_frames16_reduced(self, streams, r, outs=None, frame_stride=None):
        """streams: int16 [3 n, >= max_stream_shorts()]; returns the reduced R, G, B planes as three int16
        [n, AH >> r, AW >> r] tensors (or writes frame f's planes frame_stride BYTES behind outs[0..2], frame 0's)."""
        assert streams.stride(-1) == 1 and streams.shape[0] % 3 == 0
        n = streams.shape[0] // 3
        if outs is None:
            outs = [self.torch.empty((n, self.ah >> r, self.aw >> r), dtype=self.torch.int16, device=self.dev) for _ in range(3)]
        if frame_stride is None:
            frame_stride = 2 * outs[0].stride(0) if n > 1 else 0
        _check(self.L.picsong_decode_rgb_frames16_reduced(self.h, n, self._p(streams), streams.stride(0), r, self._p(outs[0]),
                                                          self._p(outs[1]), self._p(outs[2]), frame_stride or 0, self._stream()))
        return outs

    def decode_rgb_frames16_window(self, streams, x, y, w, h, r=0, outs=None):
        """streams: int16 [3 n, >= max_stream_shorts()]; returns the R, G, B windows as three int16 [n, h, w] tensors (or
        fills `outs`, three 3-D int16 views with the same frame stride, stride(0), and pitch, stride(1))."""
        assert streams.stride(-1) == 1 and streams.shape[0] % 3 == 0
        n = streams.shape[0] // 3
        if outs is None:
            outs = [self.torch.empty((n, h, w), dtype=self.torch.int16, device=self.dev) for _ in range(3)]
        for o in outs:
            assert o.dtype == self.torch.int16 and tuple(o.shape) == (n, h, w) and o.stride(2) == 1
            assert o.stride(0) == outs[0].stride(0) and o.stride(1) == outs[0].stride(1)
        _check(self.L.picsong_decode_rgb_frames16_window(self.h, n, self._p(streams), streams.stride(0), r, x, y, w, h, self._p(outs[0]),
                                                         self._p(outs[1]), self._p(outs[2]), 2 * outs[0].stride(1), 2 * outs[0].stride(0),
                                                         self._stream()))
        return outs

    # ---- whole frame (asynchronous; last_total() synchronises) ----
    def encode_frame_async(self, frame_u8_padded, out_stream, iter_=0):
        _check(self.L.picsong_encode_frame(self.h, self._p(frame_u8_padded), iter_, self._p(out_stream),
                                           self._stream()))

    def last_total(self):
        t = C.c_int()
        _check(self.L.picsong_last_total(self.h, self._stream(), C.byref(t)))
        return t.value

    def encode_frame(self, frame_u8_padded, iter_=0):
        out = self.torch.empty(self.max_stream_shorts(), dtype=self.torch.int16, device=self.dev)
        self.encode_frame_async(frame_u8_padded, out, iter_)
        return out[:self.last_total()]

    # ---- batched frames: n frames, one launch per stage (picsong_encode_frames) ----
    def encode_frames_async(self, frames_u8_padded, out_streams, first_iter=0):
        """frames_u8_padded: uint8 [n, AH*AW] (rows contiguous, any row stride that is a multiple of 16);
        out_streams: int16 [n, >= max_stream_shorts()]."""
        n = frames_u8_padded.shape[0]
        assert out_streams.shape[0] >= n and frames_u8_padded.stride(-1) == 1 and out_streams.stride(-1) == 1
        _check(self.L.picsong_encode_frames(self.h, n, self._p(frames_u8_padded), frames_u8_padded.stride(0),
                                            first_iter, self._p(out_streams), out_streams.stride(0), self._stream()))
        return n

    def last_totals(self, n):
        t = (C.c_int * n)()
        _check(self.L.picsong_last_totals(self.h, self._stream(), n, t))
        return list(t)

    def decode_frames(self, streams, out=None):
        """streams: int16 [n, >= max_stream_shorts()] (codestream f in row f); returns uint8 [n, AH, AW]."""
        n = streams.shape[0]
        assert streams.stride(-1) == 1
        if out is None:
            out = self.torch.empty((n, self.ah, self.aw), dtype=self.torch.uint8, device=self.dev)
        _check(self.L.picsong_decode_frames(self.h, n, self._p(streams), streams.stride(0), self._p(out), out.stride(0),
                                            self._stream()))
        return out

    def copy_last_totals(self, n, d_totals):
        """The lengths of the most recent encode_frame (n = 1) / encode_frames call into an int32 device tensor, on
        this context's stream, without a wait."""
        assert d_totals.dtype == self.torch.int32 and d_totals.numel() >= n
        _check(self.L.picsong_copy_last_totals(self.h, self._stream(), n, self._p(d_totals)))

    def encode_frames(self, frames_u8_padded, first_iter=0):
        n = frames_u8_padded.shape[0]
        out = self.torch.empty((n, self.max_stream_shorts()), dtype=self.torch.int16, device=self.dev)
        self.encode_frames_async(frames_u8_padded, out, first_iter)
        return [out[i, :t] for i, t in enumerate(self.last_totals(n))]

    def encode_frame_stripe(self, frame_u8_padded, cb_begin, cb_count):
        """Mini-stream (9 x 0xFFFF | pairs | payload | 0xFFFF) of codeblocks [cb_begin, +cb_count)."""
        out = self.torch.empty(9 + 2 * cb_count + cb_count * 4096 + 1, dtype=self.torch.int16, device=self.dev)
        _check(self.L.picsong_encode_frame_stripe(self.h, self._p(frame_u8_padded), cb_begin, cb_count,
                                                  self._p(out), self._stream()))
        return out[:self.last_total()]

    # ---- row-band sharding of the transform (intra-frame split) ----
    def new_coef_buffer(self):
        return self.torch.zeros(self.P + self.extra, dtype=self.torch.float32 if self.lossy else self.torch.int32,
                                device=self.dev)

    def dwt_forward_band(self, frame_u8_frame_coords, row0, rows, coef):
        _check(self.L.picsong_dwt_forward_band(self.h, self._p(frame_u8_frame_coords), row0, rows, self._p(coef),
                                               self._stream()))

    def dwt_forward_tail(self, coef):
        _check(self.L.picsong_dwt_forward_tail(self.h, self._p(coef), self._stream()))

    def encode_stripe_coded(self, coef, cb_begin, cb_count):
        out = self.torch.empty(9 + 2 * cb_count + cb_count * 4096 + 1, dtype=self.torch.int16, device=self.dev)
        _check(self.L.picsong_encode_stripe_coded(self.h, self._p(coef), cb_begin, cb_count, self._p(out),
                                                  self._stream()))
        return out[:self.last_total()]

    def decode_frame(self, stream):
        out = self.torch.empty(self.P, dtype=self.torch.uint8, device=self.dev)
        _check(self.L.picsong_decode_frame(self.h, self._p(stream), self._p(out), self._stream()))
        return out.view(self.ah, self.aw)

    # ---- reduced-resolution decode (1/2^r of the frame's size; r = 0 is the full decode) ----
    def reduced_dims(self, r):
        """(visible width, height, padded width, height, codeblocks decoded) of the image at 1/2^r."""
        d = [C.c_int() for _ in range(5)]
        _check(self.L.picsong_reduced_dims(self.h, r, *[C.byref(x) for x in d]))
        return tuple(x.value for x in d)

    def decode_frame_reduced(self, stream, r):
        """The padded reduced image, uint8 (AH >> r, AW >> r)."""
        out = self.torch.empty((self.ah >> r, self.aw >> r), dtype=self.torch.uint8, device=self.dev)
        _check(self.L.picsong_decode_frame_reduced(self.h, self._p(stream), r, self._p(out), self._stream()))
        return out

    def decode_frames_reduced(self, streams, r, out=None):
        """streams: int16 [n, >= max_stream_shorts()]; returns uint8 [n, AH >> r, AW >> r] (or fills `out`, whose
        frames may lie further apart)."""
        n = streams.shape[0]
        assert streams.stride(-1) == 1
        if out is None:
            out = self.torch.empty((n, self.ah >> r, self.aw >> r), dtype=self.torch.uint8, device=self.dev)
        _check(self.L.picsong_decode_frames_reduced(self.h, n, self._p(streams), streams.stride(0), r, self._p(out),
                                                    out.stride(0), self._stream()))
        return out

    def decode_rgb_frame_reduced(self, streams, r):
        """streams: int16 [3, >= max_stream_shorts()]; returns the three reduced u8 planes (AH >> r, AW >> r)."""
        outs = [self.torch.empty((self.ah >> r, self.aw >> r), dtype=self.torch.uint8, device=self.dev) for _ in range(3)]
        _check(self.L.picsong_decode_rgb_frame_reduced(self.h, self._p(streams), streams.stride(0), r, self._p(outs[0]),
                                                       self._p(outs[1]), self._p(outs[2]), self._stream()))
        return outs

    # ---- window decode: the rectangle [x, x + w) x [y, y + h) of the padded image at 1/2^r ----
    def window_codeblocks(self, x, y, w, h, r=0):
        """The codeblocks one window call decodes (per frame, per component)."""
        n = C.c_int()
        _check(self.L.picsong_window_codeblocks(self.h, r, x, y, w, h, C.byref(n)))
        return n.value

    def _window_out(self, out, h, w):
        if out is None:
            return self.torch.empty((h, w), dtype=self.torch.uint8, device=self.dev)
        assert out.dtype == self.torch.uint8 and out.dim() == 2 and tuple(out.shape) == (h, w) and out.stride(1) == 1
        return out

    def decode_frame_window(self, stream, x, y, w, h, r=0, out=None):
        """The window, uint8 (h, w); or written into `out`, a 2-D uint8 view whose row stride is the pitch."""
        out = self._window_out(out, h, w)
        _check(self.L.picsong_decode_frame_window(self.h, self._p(stream), r, x, y, w, h, self._p(out), out.stride(0),
                                                  self._stream()))
        return out

    def decode_frames_window(self, streams, x, y, w, h, r=0, out=None):
        """streams: int16 [n, >= max_stream_shorts()]; returns uint8 [n, h, w] (or fills `out`, a 3-D uint8 view:
        frame stride out.stride(0), pitch out.stride(1))."""
        n = streams.shape[0]
        assert streams.stride(-1) == 1
        if out is None:
            out = self.torch.empty((n, h, w), dtype=self.torch.uint8, device=self.dev)
        assert out.dtype == self.torch.uint8 and tuple(out.shape) == (n, h, w) and out.stride(2) == 1
        _check(self.L.picsong_decode_frames_window(self.h, n, self._p(streams), streams.stride(0), r, x, y, w, h,
                                                   self._p(out), out.stride(1), out.stride(0), self._stream()))
        return out

    def decode_rgb_frame_window(self, streams, x, y, w, h, r=0, outs=None):
        """streams: int16 [3, >= max_stream_shorts()]; returns the three u8 windows (h, w) (or fills `outs`, three 2-D
        uint8 views with the same row stride)."""
        outs = [self._window_out(None if outs is None else o, h, w) for o in (outs or [None] * 3)]
        assert outs[0].stride(0) == outs[1].stride(0) == outs[2].stride(0)
        _check(self.L.picsong_decode_rgb_frame_window(self.h, self._p(streams), streams.stride(0), r, x, y, w, h,
                                                      self._p(outs[0]), self._p(outs[1]), self._p(outs[2]),
                                                      outs[0].stride(0), self._stream()))
        return outs

    # ---- colour proxies: n RGB frames at 1/2^r, or a window of them, through one launch per stage ----
    def decode_rgb_frames_reduced(self, streams, r, outs=None, frame_stride=None):
        """streams: int16 [3 n, >= max_stream_shorts()]; returns the reduced R, G, B planes as three uint8
        [n, AH >> r, AW >> r] tensors (or writes frame f's planes frame_stride bytes behind outs[0..2], frame 0's)."""
        assert streams.stride(-1) == 1 and streams.shape[0] % 3 == 0
        n = streams.shape[0] // 3
        if outs is None:
            outs = [self.torch.empty((n, self.ah >> r, self.aw >> r), dtype=self.torch.uint8, device=self.dev) for _ in range(3)]
            frame_stride = outs[0].stride(0)
        _check(self.L.picsong_decode_rgb_frames_reduced(self.h, n, self._p(streams), streams.stride(0), r, self._p(outs[0]),
                                                        self._p(outs[1]), self._p(outs[2]), frame_stride or 0, self._stream()))
        return outs

    def decode_rgb_frames_window(self, streams, x, y, w, h, r=0, outs=None):
        """streams: int16 [3 n, >= max_stream_shorts()]; returns the R, G, B windows as three uint8 [n, h, w] tensors (or
        fills `outs`, three 3-D uint8 views with the same frame stride, stride(0), and pitch, stride(1))."""
        assert streams.stride(-1) == 1 and streams.shape[0] % 3 == 0
        n = streams.shape[0] // 3
        if outs is None:
            outs = [self.torch.empty((n, h, w), dtype=self.torch.uint8, device=self.dev) for _ in range(3)]
        for o in outs:
            assert o.dtype == self.torch.uint8 and tuple(o.shape) == (n, h, w) and o.stride(2) == 1
            assert o.stride(0) == outs[0].stride(0) and o.stride(1) == outs[0].stride(1)
        _check(self.L.picsong_decode_rgb_frames_window(self.h, n, self._p(streams), streams.stride(0), r, x, y, w, h, self._p(outs[0]),
                                                       self._p(outs[1]), self._p(outs[2]), outs[0].stride(1), outs[0].stride(0),
                                                       self._stream()))
        return outs

    def decode_rgb_images_reduced(self, streams, r, img, frame_stride=0):
        """streams: int16 [3 n, >= max_stream_shorts()]; the visible rw x rh pixels (reduced_dims) of the n frames at 1/2^r
        land in `img` (any colour layout; frame f frame_stride bytes behind frame 0), alpha (if any) 255.  A deep RGB context
        takes LAYOUT_PLANAR3_16, LAYOUT_RGB48 and LAYOUT_RGBA64 (alpha 2^bd - 1)."""
        assert streams.stride(-1) == 1 and streams.shape[0] % 3 == 0
        _check(self.L.picsong_decode_rgb_images_reduced(self.h, streams.shape[0] // 3, self._p(streams), streams.stride(0), r,
                                                        C.byref(img), frame_stride, self._stream()))

    def decode_rgb_images_window(self, streams, x, y, w, h, img, r=0, frame_stride=0):
        """... and the w x h window at (x, y) of the padded image at 1/2^r, in the layout of `img` (a deep RGB context:
        LAYOUT_PLANAR3_16, LAYOUT_RGB48 or LAYOUT_RGBA64, alpha 2^bd - 1)."""
        assert streams.stride(-1) == 1 and streams.shape[0] % 3 == 0
        _check(self.L.picsong_decode_rgb_images_window(self.h, streams.shape[0] // 3, self._p(streams), streams.stride(0), r, x, y, w,
                                                       h, C.byref(img), frame_stride, self._stream()))
