"""ctypes binding of liblfm.so (the MI355X-native .lfm encoder / decoder).

This is the same C ABI a Matlab MEX, a JNI wrapper or any other FFI caller
binds (include/lfm/*.h); Python is only a test / bench harness here.

GPU entry points need a visible gfx950 device; they raise LfmError when the
library or the device is missing (there is no CPU fallback for the predictor
stage).  When PyTorch is importable it is imported BEFORE liblfm.so is loaded,
so both share one HIP runtime (libamdhip64.so.7) in the process.
"""
import ctypes
import os

import numpy as np

try:  # one HIP runtime per process: torch's, if torch is present
    import torch  # noqa: F401
    _HAVE_TORCH = True
except Exception:  # pragma: no cover
    _HAVE_TORCH = False

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("LFM_LIB") or os.path.join(PKG_DIR, "liblfm.so")

FAMILIES = {"tiles": 0, "angle_and_space": 0, "angle": 1, "space": 2}
DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.uint32): 2, np.dtype(np.uint64): 3,
          np.dtype(np.int8): 4, np.dtype(np.int16): 5, np.dtype(np.int32): 6, np.dtype(np.int64): 7,
          np.dtype(np.float32): 8, np.dtype(np.float64): 9}
NP_OF = {v: k for k, v in DTYPES.items()}

EXPORTS = [
    # klb_Cwrapper.h
    "writeKLBstack", "writeKLBstackSlices", "readKLBheader", "readKLBstack", "readKLBstackInPlace",
    "readKLBroiInPlace",
    # lfm_api.h
    "lfm_set_family", "lfm_get_family", "lfm_version", "lfm_api_version", "writeLFMstack_c", "readLFMstack_c",
    "lfm_encoder_create", "lfm_encoder_destroy", "lfm_encoder_encode", "lfm_encoder_encode_slab",
    "lfm_merge_slabs", "lfm_free", "lfm_decode_memory", "lfm_decode_memory_roi", "lfm_set_devices", "lfm_get_devices", "lfm_default_devices",
    "lfm_encoder_encode_multi", "lfm_release_encoders", "lfm_slab_info", "lfm_place_slab", "lfm_encoder_submit",
    "lfm_encoder_submit_select", "lfm_encoder_wait", "lfm_decode_memory_device", "lfm_decode_memory_roi_device",
    "lfm_set_decode_devices", "lfm_get_decode_devices", "lfm_default_decode_devices", "lfm_release_decoders",
    "lfm_decode_shard_plan", "lfm_decode_memory_multi", "lfm_decode_memory_multi_device",
    "lfm_set_bzip2_multiblock", "lfm_get_bzip2_multiblock", "lfm_encoder_stream_counts",
    "lfm_set_bunzip2_multiblock", "lfm_get_bunzip2_multiblock",
    "lfm_set_bunzip2_periodic", "lfm_get_bunzip2_periodic",
    "lfm_writer_open", "lfm_writer_axis", "lfm_writer_append", "lfm_writer_close", "lfm_writer_abort",
    "lfm_reader_open", "lfm_reader_info", "lfm_reader_read", "lfm_reader_bytes_read", "lfm_reader_close",
    "lfm_writer_flush", "lfm_recover", "lfm_reader_open_live", "lfm_reader_refresh",
    # lfm_hip.h
    "lfm_hip_predict", "lfm_hip_unpredict", "lfm_hip_unpredict_async", "lfm_hip_unpredict_check",
    "lfm_hip_unpredict_path", "lfm_hip_predict_plan", "lfm_hip_predict_set_pieces",
    "lfm_hip_predict_candidates", "lfm_hip_entropy2d", "lfm_hip_entropy2d_hist", "lfm_hip_select_workspace_bytes",
    "lfm_hip_select",
    "lfm_hip_synth", "lfm_hip_device_count", "lfm_hip_force_generic", "lfm_hip_bzip2_workspace_bytes", "lfm_hip_bzip2_out_cap",
    "lfm_hip_bzip2_blocks", "lfm_hip_bzip2_last_stage_ms", "lfm_hip_bunzip2_workspace_bytes", "lfm_hip_bunzip2_blocks", "lfm_hip_scatter_blocks",
    "lfm_hip_crop_region", "lfm_hip_bzip2_workspace_bytes_multi", "lfm_hip_bzip2_max_count_multi",
    "lfm_hip_bzip2_blocks_multi", "lfm_hip_bzip2_last_blocks", "lfm_hip_bzip2_last_bwt_stats",
    "lfm_hip_bzip2_last_place_path", "lfm_hip_bzip2_last_sort_jobs",
    "lfm_hip_bunzip2_max_parts", "lfm_hip_bunzip2_workspace_bytes_multi", "lfm_hip_bunzip2_blocks_multi",
    "lfm_hip_bunzip2_issue_multi", "lfm_hip_bunzip2_set_periodic", "lfm_hip_bunzip2_get_periodic",
]


class LfmError(RuntimeError):
    pass


class EncodeStats(ctypes.Structure):
    _fields_ = [("total_ms", ctypes.c_double), ("h2d_ms", ctypes.c_double), ("select_ms", ctypes.c_double),
                ("predict_ms", ctypes.c_double), ("d2h_ms", ctypes.c_double), ("compress_ms", ctypes.c_double),
                ("chosen", ctypes.c_int), ("header_version", ctypes.c_int), ("entropy", ctypes.c_float * 8),
                ("out_bytes", ctypes.c_uint64), ("bz_stage_ms", ctypes.c_double * 5), ("bz_in_bytes", ctypes.c_uint64)]
    BZ_STAGES = ("rle1", "bwt", "mtf", "huffman", "emit")

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_ if f not in ("entropy", "bz_stage_ms")}
        d["entropy"] = list(self.entropy)
        d["bz_stage_ms"] = dict(zip(self.BZ_STAGES, list(self.bz_stage_ms)))
        return d


class PredictLaunch(ctypes.Structure):
    """lfm_predict_launch (lfm_hip.h)."""
    _fields_ = [(f, ctypes.c_int) for f in (
        "kernel", "first", "nframes", "pairs", "strip", "nstrip", "rows_per_step", "rows_per_piece", "npiece", "R",
        "RP", "halo", "xcd_map", "grid_x", "grid_y", "threads", "lds_bytes")]


class DecodeStats(ctypes.Structure):
    """lfm_decode_stats (lfm_api.h)."""
    _fields_ = [("total_ms", ctypes.c_double), ("path", ctypes.c_int), ("chunks", ctypes.c_uint32),
                ("blocks", ctypes.c_uint64), ("host_blocks", ctypes.c_uint64), ("d2h_bytes", ctypes.c_uint64),
                ("staged_bytes", ctypes.c_uint64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class DecodeShard(ctypes.Structure):
    """lfm_decode_shard (lfm_api.h)."""
    _fields_ = [("first", ctypes.c_uint32), ("count", ctypes.c_uint32), ("device", ctypes.c_int), ("rc", ctypes.c_int),
                ("stats", DecodeStats)]

    def as_dict(self):
        return dict(first=self.first, count=self.count, device=self.device, rc=self.rc, stats=self.stats.as_dict())


class DecodeMultiStats(ctypes.Structure):
    """lfm_decode_multi_stats (lfm_api.h)."""
    _fields_ = [("total_ms", ctypes.c_double), ("axis", ctypes.c_int), ("workers", ctypes.c_int),
                ("blocks", ctypes.c_uint64), ("host_blocks", ctypes.c_uint64), ("d2h_bytes", ctypes.c_uint64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class WriterStats(ctypes.Structure):
    """lfm_writer_stats (lfm_api.h)."""
    _fields_ = [("appended", ctypes.c_uint64), ("ranges", ctypes.c_uint64), ("streams", ctypes.c_uint64),
                ("host_streams", ctypes.c_uint64), ("bzip2_blocks", ctypes.c_uint64),
                ("bytes_written", ctypes.c_uint64), ("moved_bytes", ctypes.c_uint64),
                ("staged_peak_bytes", ctypes.c_uint64), ("chosen", ctypes.c_int), ("header_version", ctypes.c_int),
                ("entropy", ctypes.c_float * 8), ("total_ms", ctypes.c_double), ("committed", ctypes.c_uint64)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_ if f != "entropy"}
        d["entropy"] = list(self.entropy)
        return d


class RecoverStats(ctypes.Structure):
    """lfm_recover_stats (lfm_api.h)."""
    _fields_ = [("axis", ctypes.c_int), ("header_version", ctypes.c_int), ("already_valid", ctypes.c_int),
                ("capacity", ctypes.c_uint64), ("kept", ctypes.c_uint64), ("committed_blocks", ctypes.c_uint64),
                ("dropped_layers", ctypes.c_uint64), ("verified_streams", ctypes.c_uint64),
                ("host_streams", ctypes.c_uint64), ("bytes_written", ctypes.c_uint64),
                ("moved_bytes", ctypes.c_uint64), ("total_ms", ctypes.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LfmError("liblfm.so is not built (run `make -C %s` or __graft_entry__.build())" % PKG_DIR)
    L = ctypes.CDLL(LIB_PATH)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    f32p = ctypes.POINTER(ctypes.c_float)
    vp = ctypes.c_void_p
    L.writeKLBstack.argtypes = [vp, ctypes.c_char_p, u32p, ctypes.c_int, ctypes.c_int, f32p, u32p, ctypes.c_int,
                                ctypes.c_char_p]
    L.writeKLBstackSlices.argtypes = [ctypes.POINTER(vp), ctypes.c_char_p, u32p, ctypes.c_int, ctypes.c_int, f32p,
                                      u32p, ctypes.c_int, ctypes.c_char_p]
    L.readKLBheader.argtypes = [ctypes.c_char_p, u32p, ctypes.POINTER(ctypes.c_int), f32p, u32p,
                                ctypes.POINTER(ctypes.c_int), ctypes.c_char_p]
    L.readKLBstack.restype = vp
    L.readKLBstack.argtypes = [ctypes.c_char_p, u32p, ctypes.POINTER(ctypes.c_int), ctypes.c_int, f32p, u32p,
                               ctypes.POINTER(ctypes.c_int), ctypes.c_char_p]
    L.readKLBstackInPlace.argtypes = [ctypes.c_char_p, vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    L.readKLBroiInPlace.argtypes = [ctypes.c_char_p, vp, u32p, u32p, ctypes.c_int]
    L.lfm_version.restype = ctypes.c_char_p
    # lfm_decode_memory_roi's argument list (lfm_api.h); a library without the
    # version symbol is a round-5 build, whose list is the same
    if hasattr(L, "lfm_api_version") and L.lfm_api_version() != 2:
        raise OSError("liblfm.so API version %d, this binding needs 2" % L.lfm_api_version())
    L.writeLFMstack_c.argtypes = [vp, ctypes.c_char_p, u32p, ctypes.c_int, ctypes.c_int, f32p, u32p, ctypes.c_int,
                                  ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.readLFMstack_c.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint8),
                                 ctypes.POINTER(ctypes.c_uint8)]
    L.lfm_encoder_create.restype = vp
    L.lfm_encoder_create.argtypes = [ctypes.c_int, ctypes.c_int]
    L.lfm_encoder_destroy.argtypes = [vp]
    L.lfm_encoder_encode.argtypes = [vp, vp, ctypes.c_int, u32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, u32p,
                                     ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)),
                                     ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(EncodeStats)]
    L.lfm_encoder_encode_slab.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_uint32, u32p, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, u32p, ctypes.c_int, ctypes.c_char_p,
                                          ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)),
                                          ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(EncodeStats)]
    L.lfm_encoder_submit.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_uint32, u32p, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, u32p, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]
    L.lfm_encoder_submit_select.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_uint32, vp, u32p, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, u32p, ctypes.c_int, ctypes.c_char_p,
                                            ctypes.POINTER(ctypes.c_uint64)]
    L.lfm_encoder_wait.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)),
                                   ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(EncodeStats)]
    L.lfm_encoder_encode_multi.argtypes = [vp, vp, u32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, u32p,
                                           ctypes.c_int, ctypes.c_char_p,
                                           ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)),
                                           ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(EncodeStats)]
    L.lfm_slab_info.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.lfm_place_slab.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64,
                                 ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
    L.lfm_set_devices.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    L.lfm_get_devices.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    L.lfm_default_devices.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    L.lfm_release_encoders.argtypes = []
    L.lfm_release_encoders.restype = None
    L.lfm_merge_slabs.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint64), ctypes.c_int,
                                  ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), ctypes.POINTER(ctypes.c_uint64)]
    L.lfm_free.argtypes = [vp]
    L.lfm_free.restype = None
    L.lfm_decode_memory.argtypes = [ctypes.c_char_p, ctypes.c_uint64, vp, ctypes.c_int]
    L.lfm_decode_memory_roi.argtypes = [vp, ctypes.c_uint64, u32p, u32p, vp, ctypes.c_uint64, ctypes.c_int]
    L.lfm_hip_predict.argtypes = [vp, vp, vp] + [ctypes.c_int] * 8 + [vp]
    L.lfm_hip_unpredict.argtypes = [vp, vp, vp] + [ctypes.c_int] * 8 + [vp]
    L.lfm_hip_unpredict_async.argtypes = [vp, vp, vp] + [ctypes.c_int] * 8 + [vp, vp]
    L.lfm_hip_unpredict_check.argtypes = [ctypes.c_int]
    L.lfm_hip_predict_candidates.argtypes = [vp, vp] + [ctypes.c_int] * 4 + [vp]
    L.lfm_hip_entropy2d.argtypes = [vp, ctypes.c_uint64, f32p, vp]
    L.lfm_hip_entropy2d_hist.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_uint64, vp, vp]
    L.lfm_hip_bzip2_workspace_bytes.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.lfm_hip_bzip2_workspace_bytes.restype = ctypes.c_size_t
    L.lfm_hip_bzip2_out_cap.argtypes = [ctypes.c_uint32]
    L.lfm_hip_bzip2_out_cap.restype = ctypes.c_size_t
    L.lfm_hip_bzip2_blocks.argtypes = [vp, u32p, u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                       ctypes.c_uint32, vp, ctypes.c_size_t, vp,
                                       ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), vp]
    L.lfm_hip_bzip2_workspace_bytes_multi.argtypes = [ctypes.c_uint32] * 3
    L.lfm_hip_bzip2_workspace_bytes_multi.restype = ctypes.c_size_t
    L.lfm_hip_bzip2_max_count_multi.argtypes = [ctypes.c_uint32] * 2
    L.lfm_hip_bzip2_max_count_multi.restype = ctypes.c_uint32
    L.lfm_hip_bzip2_blocks_multi.argtypes = L.lfm_hip_bzip2_blocks.argtypes
    L.lfm_hip_bzip2_last_blocks.argtypes = []
    L.lfm_hip_bzip2_last_blocks.restype = ctypes.c_uint64
    L.lfm_hip_bzip2_last_bwt_stats.argtypes = [u32p]
    L.lfm_hip_bzip2_last_bwt_stats.restype = None
    L.lfm_hip_bzip2_last_sort_jobs.argtypes = [u32p]
    L.lfm_hip_bzip2_last_sort_jobs.restype = None
    L.lfm_hip_bzip2_last_place_path.argtypes = []
    L.lfm_hip_bzip2_last_place_path.restype = ctypes.c_uint32
    L.lfm_set_bzip2_multiblock.argtypes = [ctypes.c_int]
    L.lfm_get_bzip2_multiblock.argtypes = []
    L.lfm_encoder_stream_counts.argtypes = [vp] + [ctypes.POINTER(ctypes.c_uint64)] * 3
    L.lfm_hip_bunzip2_workspace_bytes.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.lfm_hip_bunzip2_workspace_bytes.restype = ctypes.c_size_t
    L.lfm_hip_bunzip2_blocks.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, vp, ctypes.c_uint32,
                                         vp, ctypes.c_size_t, u32p, u32p, vp]
    L.lfm_hip_bunzip2_max_parts.argtypes = [ctypes.c_uint32] * 2
    L.lfm_hip_bunzip2_max_parts.restype = ctypes.c_uint32
    L.lfm_hip_bunzip2_workspace_bytes_multi.argtypes = [ctypes.c_uint32] * 3
    L.lfm_hip_bunzip2_workspace_bytes_multi.restype = ctypes.c_size_t
    L.lfm_hip_bunzip2_blocks_multi.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, vp,
                                               ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_size_t, u32p, u32p, vp]
    L.lfm_set_bunzip2_multiblock.argtypes = [ctypes.c_int]
    L.lfm_get_bunzip2_multiblock.argtypes = []
    L.lfm_set_bunzip2_periodic.argtypes = [ctypes.c_int]
    L.lfm_get_bunzip2_periodic.argtypes = []
    L.lfm_hip_scatter_blocks.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p,
                                         ctypes.c_uint32, vp, vp]
    L.lfm_hip_select_workspace_bytes.restype = ctypes.c_size_t
    L.lfm_hip_select_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    L.lfm_hip_select.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, f32p,
                                 ctypes.POINTER(ctypes.c_int), vp, vp]
    L.lfm_hip_synth.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, vp]
    # the device-destination readers and the region copy: a library built
    # before them still loads for everything else
    if hasattr(L, "lfm_decode_memory_device"):
        L.lfm_decode_memory_device.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_int,
                                               ctypes.POINTER(DecodeStats)]
    if hasattr(L, "lfm_decode_memory_roi_device"):
        L.lfm_decode_memory_roi_device.argtypes = [vp, ctypes.c_uint64, u32p, u32p, vp, ctypes.c_uint64, ctypes.c_int,
                                                   ctypes.POINTER(DecodeStats)]
    if hasattr(L, "lfm_hip_crop_region"):
        L.lfm_hip_crop_region.argtypes = [vp, u32p, u32p, u32p, ctypes.c_uint32, vp, vp]
    if hasattr(L, "lfm_hip_unpredict_path"):
        L.lfm_hip_unpredict_path.argtypes = [ctypes.c_int] * 3
    if hasattr(L, "lfm_hip_predict_plan"):
        L.lfm_hip_predict_plan.argtypes = [ctypes.c_int] * 10 + [ctypes.POINTER(PredictLaunch), ctypes.c_int]
        L.lfm_hip_predict_set_pieces.argtypes = [ctypes.c_int]
    # the multi-GPU reader, likewise
    intp = ctypes.POINTER(ctypes.c_int)
    if hasattr(L, "lfm_set_decode_devices"):
        L.lfm_set_decode_devices.argtypes = [intp, ctypes.c_int]
    if hasattr(L, "lfm_get_decode_devices"):
        L.lfm_get_decode_devices.argtypes = [intp, ctypes.c_int]
    if hasattr(L, "lfm_default_decode_devices"):
        L.lfm_default_decode_devices.argtypes = [ctypes.c_int, intp, ctypes.c_int]
    if hasattr(L, "lfm_release_decoders"):
        L.lfm_release_decoders.argtypes = []
        L.lfm_release_decoders.restype = None
    if hasattr(L, "lfm_decode_shard_plan"):
        L.lfm_decode_shard_plan.argtypes = [vp, ctypes.c_uint64, ctypes.c_int, intp, u32p, u32p, ctypes.c_int]
    if hasattr(L, "lfm_decode_memory_multi"):
        L.lfm_decode_memory_multi.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_int,
                                              ctypes.POINTER(DecodeMultiStats), ctypes.POINTER(DecodeShard),
                                              ctypes.c_int]
    if hasattr(L, "lfm_decode_memory_multi_device"):
        L.lfm_decode_memory_multi_device.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(vp),
                                                     ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.c_int,
                                                     ctypes.POINTER(DecodeMultiStats), ctypes.POINTER(DecodeShard),
                                                     ctypes.c_int]
    # the stream writer and the ranged reader, likewise
    if hasattr(L, "lfm_writer_open"):
        L.lfm_writer_open.argtypes = [ctypes.POINTER(vp), ctypes.c_char_p, u32p, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, f32p, u32p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int,
                                      ctypes.c_int]
        L.lfm_writer_axis.argtypes = [vp]
        L.lfm_writer_append.argtypes = [vp, vp, ctypes.c_int, ctypes.c_uint32]
        L.lfm_writer_close.argtypes = [vp, ctypes.POINTER(WriterStats)]
        L.lfm_writer_abort.argtypes = [vp]
        L.lfm_writer_abort.restype = None
    if hasattr(L, "lfm_reader_open"):
        L.lfm_reader_open.argtypes = [ctypes.POINTER(vp), ctypes.c_char_p]
        L.lfm_reader_info.argtypes = [vp, u32p, intp, u32p, ctypes.POINTER(ctypes.c_uint8),
                                      ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)]
        L.lfm_reader_read.argtypes = [vp, u32p, u32p, vp, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(DecodeStats)]
        L.lfm_reader_bytes_read.argtypes = [vp]
        L.lfm_reader_bytes_read.restype = ctypes.c_uint64
        L.lfm_reader_close.argtypes = [vp]
        L.lfm_reader_close.restype = None
    # checkpoints, recovery and the live reader, likewise
    if hasattr(L, "lfm_writer_flush"):
        L.lfm_writer_flush.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
    if hasattr(L, "lfm_recover"):
        L.lfm_recover.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                  ctypes.POINTER(RecoverStats)]
    if hasattr(L, "lfm_reader_open_live"):
        L.lfm_reader_open_live.argtypes = [ctypes.POINTER(vp), ctypes.c_char_p]
    if hasattr(L, "lfm_reader_refresh"):
        L.lfm_reader_refresh.argtypes = [vp, u32p]
    _lib = L
    return L


def missing_exports():
    L = lib()
    return [name for name in EXPORTS if not hasattr(L, name)]


def device_count():
    return int(lib().lfm_hip_device_count())


def require_gpu():
    if device_count() <= 0:
        raise LfmError("no HIP device visible: the LFM predictor stage runs only on the GPU")


def set_devices(devices=None):
    """Devices the writers farm block ranges to (lfm_set_devices); None or []
    restores the default (see default_devices)."""
    devices = list(devices or [])
    arr = (ctypes.c_int * max(1, len(devices)))(*devices)
    _check(lib().lfm_set_devices(arr, len(devices)), "lfm_set_devices")


def get_devices():
    arr = (ctypes.c_int * 256)()
    n = lib().lfm_get_devices(arr, 256)
    return list(arr[:min(n, 256)])


def default_devices(n_visible, current=-1):
    """The writers' default device list on a machine with n_visible devices
    (lfm_default_devices: env LFM_GPUS / LOCAL_WORLD_SIZE / LOCAL_RANK / ...;
    no device call)."""
    arr = (ctypes.c_int * 256)()
    n = lib().lfm_default_devices(int(n_visible), int(current), arr, 256)
    return list(arr[:min(n, 256)])


def release_encoders():
    """Free the device / pinned buffers the writers keep between calls."""
    lib().lfm_release_encoders()


def set_family(family):
    if lib().lfm_set_family(FAMILIES.get(family, family)) != 0:
        raise LfmError("bad family %r" % (family,))


def get_family():
    return int(lib().lfm_get_family())


def _u32(v):
    return (ctypes.c_uint32 * 5)(*[int(x) for x in v])


def _f32(v):
    return (ctypes.c_float * 5)(*[float(x) for x in v])


def _xyzct(arr):
    a = arr
    while a.ndim < 5:
        a = a[None]
    t, c, z, y, x = a.shape
    return [x, y, z, c, t]


def _meta(m):
    if m is None:
        return None
    b = m.encode() if isinstance(m, str) else bytes(m)
    return ctypes.create_string_buffer(b[:256].ljust(256, b"\0"), 256)


def _check(rc, what):
    if rc != 0:
        raise LfmError("%s failed with code %d" % (what, rc))


# ------------------------------------------------------------- file API --
def write_lfm(path, img, predictor_request=0, nnum=13, video=0, block_size=None, pixel_size=None,
              compression=1, metadata=None, num_threads=-1, family=None):
    """MEX writeLFMstack semantics.  img: ndarray indexed [t, c, z, y, x] (or fewer leading dims)."""
    img = np.ascontiguousarray(img)
    if family is not None:
        set_family(family)
    xyzct = _xyzct(img)
    rc = lib().writeLFMstack_c(img.ctypes.data, os.fsencode(path), _u32(xyzct), DTYPES[img.dtype], num_threads,
                               _f32(pixel_size) if pixel_size is not None else None,
                               _u32(block_size) if block_size is not None else None, compression, _meta(metadata),
                               int(predictor_request), int(nnum), int(video))
    _check(rc, "writeLFMstack_c")


def write_klb(path, img, block_size=None, pixel_size=None, compression=1, metadata=None, num_threads=-1):
    """writeKLBstack (C ABI): headerVersion 0 (auto predictor), Nnum 13."""
    img = np.ascontiguousarray(img)
    rc = lib().writeKLBstack(img.ctypes.data, os.fsencode(path), _u32(_xyzct(img)), DTYPES[img.dtype], num_threads,
                             _f32(pixel_size) if pixel_size is not None else None,
                             _u32(block_size) if block_size is not None else None, compression, _meta(metadata))
    _check(rc, "writeKLBstack")


def read_header(path):
    xyzct = (ctypes.c_uint32 * 5)()
    dt = ctypes.c_int()
    ps = (ctypes.c_float * 5)()
    bs = (ctypes.c_uint32 * 5)()
    ct = ctypes.c_int()
    md = ctypes.create_string_buffer(256)
    _check(lib().readKLBheader(os.fsencode(path), xyzct, ctypes.byref(dt), ps, bs, ctypes.byref(ct), md),
           "readKLBheader")
    return dict(xyzct=list(xyzct), data_type=dt.value, pixel_size=list(ps), block_size=list(bs),
                compression=ct.value, metadata=md.raw)


def read_lfm(path, num_threads=-1, family=None):
    """Decode a .lfm file; returns (ndarray [t, c, z, y, x], header_version, nnum)."""
    if family is not None:
        set_family(family)
    h = read_header(path)
    x, y, z, c, t = h["xyzct"]
    out = np.empty((t, c, z, y, x), dtype=NP_OF[h["data_type"]])
    hv = ctypes.c_uint8()
    nn = ctypes.c_uint8()
    _check(lib().readLFMstack_c(os.fsencode(path), out.ctypes.data, num_threads, ctypes.byref(hv), ctypes.byref(nn)),
           "readLFMstack_c")
    return out, hv.value, nn.value


# ------------------------------------------------------ in-memory encoder --
class Encoder:
    """lfm_encoder: encode host arrays or device-resident tensors to .lfm bytes."""

    def __init__(self, device=-1, num_threads=-1):
        if device < 0 and _HAVE_TORCH and torch.cuda.is_available():
            device = torch.cuda.current_device()
        self._device = device
        self._h = lib().lfm_encoder_create(device, num_threads)
        if not self._h:
            raise LfmError("lfm_encoder_create failed")

    def close(self):
        if self._h:
            lib().lfm_encoder_destroy(self._h)
            self._h = None

    def stream_counts(self):
        """How the bzip2 streams of the last encode()/encode_slab()/wait() on
        this encoder were compressed: {"streams", "host_streams" (by the host
        library), "bzip2_blocks" (bzip2 blocks the GPU produced)}.  All 0 after
        encode_multi(), which encodes on other encoders."""
        v = [ctypes.c_uint64() for _ in range(3)]
        _check(lib().lfm_encoder_stream_counts(self._h, *[ctypes.byref(x) for x in v]), "lfm_encoder_stream_counts")
        return {"streams": v[0].value, "host_streams": v[1].value, "bzip2_blocks": v[2].value}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    _TORCH_KLB = {"torch.uint8": 0, "torch.uint16": 1, "torch.int16": 1, "torch.uint32": 2, "torch.uint64": 3,
                  "torch.int8": 4, "torch.int32": 6, "torch.int64": 7, "torch.float32": 8, "torch.float64": 9}

    def _operand(self, img, xyzct, data_type):
        """(pointer, is_device, xyzct, data_type, keepalive) of a numpy array or torch tensor.
        A CUDA tensor must be contiguous and live on this encoder's device;
        int16 is taken as a uint16 view (torch has no uint16 arithmetic)."""
        if _HAVE_TORCH and isinstance(img, torch.Tensor):
            if img.is_cuda:
                if not img.is_contiguous():
                    raise LfmError("device input must be contiguous (got strides %s)" % (img.stride(),))
                if self._device >= 0 and img.device.index != self._device:
                    raise LfmError("device input lives on cuda:%d, the encoder on cuda:%d"
                                   % (img.device.index, self._device))
                kt = self._TORCH_KLB.get(str(img.dtype))
                if kt is None:
                    raise LfmError("unsupported tensor dtype %s" % img.dtype)
                if data_type is not None and data_type != kt and not (data_type == 1 and kt in (1, 5)):
                    raise LfmError("data_type %d does not match tensor dtype %s" % (data_type, img.dtype))
                # the library orders its reads after the null stream's work
                # (torch's default stream); a producer on another current
                # stream is waited for here
                cur = torch.cuda.current_stream(img.device)
                if cur != torch.cuda.default_stream(img.device):
                    cur.synchronize()
                shape = list(img.shape)
                while len(shape) < 5:
                    shape = [1] + shape
                xyzct = xyzct or [shape[4], shape[3], shape[2], shape[1], shape[0]]
                return img.data_ptr(), 1, xyzct, (kt if data_type is None else data_type), img
            img = img.numpy()
        img = np.ascontiguousarray(img)
        xyzct = xyzct or _xyzct(img)
        data_type = DTYPES[img.dtype] if data_type is None else data_type
        return img.ctypes.data, 0, xyzct, data_type, img

    def encode(self, img, header_version=0, nnum=13, block_size=None, compression=1, metadata=None,
               xyzct=None, data_type=None, copy=True):
        """img: numpy array [t,c,z,y,x] (host) or a torch CUDA tensor (device, uint16 viewed as int16 ok).
        Returns (.lfm, stats dict): bytes, or with copy=False a zero-copy
        memoryview of the encoder's buffer, valid until its next call."""
        ptr, dev, xyzct, data_type, keep = self._operand(img, xyzct, data_type)
        out = ctypes.POINTER(ctypes.c_uint8)()
        n = ctypes.c_uint64()
        st = EncodeStats()
        rc = lib().lfm_encoder_encode(self._h, ptr, dev, _u32(xyzct), data_type, int(header_version), int(nnum),
                                      _u32(block_size) if block_size is not None else None, compression,
                                      _meta(metadata), ctypes.byref(out), ctypes.byref(n), ctypes.byref(st))
        _check(rc, "lfm_encoder_encode")
        del keep
        if not copy:
            return memoryview((ctypes.c_uint8 * n.value).from_address(ctypes.addressof(out.contents))), st.as_dict()
        return ctypes.string_at(out, n.value), st.as_dict()

    def submit(self, img, z0=0, prev=None, header_version=0, nnum=13, block_size=None, compression=1,
               metadata=None, xyzct=None, data_type=None, select_frame=None):
        """Pipelined encode (lfm_encoder_submit) of a stack (z0 = 0) or a z-slab:
        returns a ticket once every kernel has run (img may be released); the
        .lfm's last payload copies finish in the background.  wait(ticket)
        gives (.lfm, stats); at most two encodes are in flight.
        select_frame: the frame auto-selection runs on (the whole stack's frame
        0 for a slab; lfm_encoder_submit_select), same residency as img."""
        ptr, dev, xyzct, data_type, keep = self._operand(img, xyzct, data_type)
        pptr = None
        if prev is not None:
            pptr, pdev, _, _, pkeep = self._operand(prev, [1, 1, 1, 1, 1], data_type)
            if pdev != dev:
                raise LfmError("prev must live where img lives (host or device)")
        sptr = None
        if select_frame is not None:
            sptr, sdev, _, _, skeep = self._operand(select_frame, [1, 1, 1, 1, 1], data_type)
            if sdev != dev:
                raise LfmError("select_frame must live where img lives (host or device)")
        t = ctypes.c_uint64()
        rc = lib().lfm_encoder_submit_select(self._h, ptr, dev, pptr, int(z0), sptr, _u32(xyzct), data_type,
                                             int(header_version), int(nnum),
                                             _u32(block_size) if block_size is not None else None, compression,
                                             _meta(metadata), ctypes.byref(t))
        _check(rc, "lfm_encoder_submit_select")
        del keep
        return t.value

    def wait(self, ticket, copy=True):
        """(.lfm, stats) of a submitted encode; with copy=False a zero-copy
        memoryview valid until the second submit after it."""
        out = ctypes.POINTER(ctypes.c_uint8)()
        n = ctypes.c_uint64()
        st = EncodeStats()
        rc = lib().lfm_encoder_wait(self._h, ticket, ctypes.byref(out), ctypes.byref(n), ctypes.byref(st))
        _check(rc, "lfm_encoder_wait")
        if not copy:
            return memoryview((ctypes.c_uint8 * n.value).from_address(ctypes.addressof(out.contents))), st.as_dict()
        return ctypes.string_at(out, n.value), st.as_dict()

    def encode_multi(self, img, header_version=0, nnum=13, block_size=None, compression=1, metadata=None,
                     data_type=None, copy=True):
        """Encode a HOST stack on every device of set_devices() (the multi-GPU
        block scheduler behind klb_imageIO::writeImage).  Returns (.lfm, stats)."""
        img = np.ascontiguousarray(img)
        xyzct = _xyzct(img)
        data_type = DTYPES[img.dtype] if data_type is None else data_type
        out = ctypes.POINTER(ctypes.c_uint8)()
        n = ctypes.c_uint64()
        st = EncodeStats()
        rc = lib().lfm_encoder_encode_multi(self._h, img.ctypes.data, _u32(xyzct), data_type, int(header_version),
                                            int(nnum), _u32(block_size) if block_size is not None else None,
                                            compression, _meta(metadata), ctypes.byref(out), ctypes.byref(n),
                                            ctypes.byref(st))
        _check(rc, "lfm_encoder_encode_multi")
        if not copy:
            return memoryview((ctypes.c_uint8 * n.value).from_address(ctypes.addressof(out.contents))), st.as_dict()
        return ctypes.string_at(out, n.value), st.as_dict()

    def encode_slab(self, img, z0, prev=None, header_version=8, nnum=13, block_size=None, compression=1,
                    metadata=None, xyzct=None, data_type=None, copy=True):
        """Encode the z-slab of a larger stack that starts at global frame z0
        (see lfm_encoder_encode_slab); prev = raw frame z0-1 (same residency
        as img), needed when the slab starts at an odd frame of a video stack.
        Returns (slab .lfm bytes, stats)."""
        ptr, dev, xyzct, data_type, keep = self._operand(img, xyzct, data_type)
        pptr = None
        if prev is not None:
            pptr, pdev, _, _, pkeep = self._operand(prev, [1, 1, 1, 1, 1], data_type)
            if pdev != dev:
                raise LfmError("prev must live where img lives (host or device)")
        out = ctypes.POINTER(ctypes.c_uint8)()
        n = ctypes.c_uint64()
        st = EncodeStats()
        rc = lib().lfm_encoder_encode_slab(self._h, ptr, dev, pptr, int(z0), _u32(xyzct), data_type,
                                           int(header_version), int(nnum),
                                           _u32(block_size) if block_size is not None else None, compression,
                                           _meta(metadata), ctypes.byref(out), ctypes.byref(n), ctypes.byref(st))
        _check(rc, "lfm_encoder_encode_slab")
        del keep
        if not copy:
            return memoryview((ctypes.c_uint8 * n.value).from_address(ctypes.addressof(out.contents))), st.as_dict()
        return ctypes.string_at(out, n.value), st.as_dict()


def merge_slabs(slabs):
    """Join the .lfm bytes of consecutive z-slabs into the whole stack's .lfm."""
    n = len(slabs)
    arr = (ctypes.c_char_p * n)(*[bytes(b) for b in slabs])
    lens = (ctypes.c_uint64 * n)(*[len(b) for b in slabs])
    out = ctypes.POINTER(ctypes.c_uint8)()
    ln = ctypes.c_uint64()
    _check(lib().lfm_merge_slabs(arr, lens, n, ctypes.byref(out), ctypes.byref(ln)), "lfm_merge_slabs")
    try:
        return ctypes.string_at(out, ln.value)
    finally:
        lib().lfm_free(out)


def _addr(buf):
    """Address of a bytes / memoryview / numpy buffer (kept alive by the caller)."""
    if isinstance(buf, np.ndarray):
        return buf.ctypes.data
    if isinstance(buf, bytes):
        return ctypes.cast(ctypes.c_char_p(buf), ctypes.c_void_p).value
    return np.frombuffer(buf, dtype=np.uint8).ctypes.data


def slab_info(slab):
    """(payload bytes, block count) of a slab .lfm (what multi-process ranks exchange)."""
    pb, nb = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().lfm_slab_info(_addr(slab), len(slab), ctypes.byref(pb), ctypes.byref(nb)), "lfm_slab_info")
    return pb.value, nb.value


def place_slab(slab, dst, total_z, total_blocks, block_index, payload_offset, num_threads=-1):
    """Place one rank's z-slab .lfm into the whole stack's .lfm buffer `dst`
    (a writable numpy uint8 array, e.g. over shared memory) -- lfm_place_slab."""
    _check(lib().lfm_place_slab(_addr(slab), len(slab), dst.ctypes.data, dst.nbytes, int(total_z), int(total_blocks),
                                int(block_index), int(payload_offset), num_threads), "lfm_place_slab")


def decode(buf, shape_tczyx=None, dtype=np.uint16, num_threads=-1):
    if shape_tczyx is None:
        import struct
        xyzct = struct.unpack_from("<5I", buf, 2)
        dtype = NP_OF[int(np.frombuffer(buf, dtype=np.uint8, count=43)[42])]
        shape_tczyx = (xyzct[4], xyzct[3], xyzct[2], xyzct[1], xyzct[0])
    out = np.empty(shape_tczyx, dtype=dtype)
    _check(lib().lfm_decode_memory(buf, len(buf), out.ctypes.data, num_threads), "lfm_decode_memory")
    return out


def decode_roi(buf, lb, ub, dtype=None, num_threads=-1, out=None):
    """Region lb .. ub (inclusive, [x, y, z, c, t]) of an in-memory .lfm
    (lfm_decode_memory_roi); returns an array [t, c, z, y, x] of the region in
    the file's data type (header byte 42).  `dtype`, when given, must be that
    type.  `out` (optional): a C-contiguous array of the region's size and the
    file's dtype to decode into (readKLBroiInPlace's caller-owned buffer),
    returned reshaped.  The library checks the byte count as well."""
    if len(buf) < 43:
        raise ValueError("decode_roi: %d bytes hold no .lfm header" % len(buf))
    dt = int(np.frombuffer(buf, dtype=np.uint8, count=43)[42])  # (buf may be bytes, a numpy array or a memoryview)
    if dt not in NP_OF:
        raise ValueError("decode_roi: unknown data type %d in the header" % dt)
    fdt = np.dtype(NP_OF[dt])
    if dtype is not None and np.dtype(dtype) != fdt:
        raise ValueError("decode_roi: the file holds %s, not %s" % (fdt, np.dtype(dtype)))
    shape = tuple(int(u) - int(l) + 1 for l, u in zip(lb, ub))[::-1]
    if out is None:
        out = np.empty(shape, dtype=fdt)
    else:
        if not isinstance(out, np.ndarray) or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError("decode_roi: out must be a writeable C-contiguous numpy array")
        if out.dtype != fdt or out.size != int(np.prod(shape)):
            raise ValueError("decode_roi: out holds %d x %s, the region is %s x %s" % (out.size, out.dtype, shape, fdt))
        out = out.reshape(shape)
    _check(lib().lfm_decode_memory_roi(_addr(buf), len(buf), _u32(lb), _u32(ub), out.ctypes.data, out.nbytes,
                                       num_threads), "lfm_decode_memory_roi")
    return out


# --------------------------------------------------- device destinations --
_KLB_TORCH = {0: "uint8", 1: "uint16", 2: "uint32", 3: "uint64", 4: "int8", 5: "int16", 6: "int32", 7: "int64",
              8: "float32", 9: "float64"}


def _need(name):
    L = lib()
    if not hasattr(L, name):
        raise LfmError("liblfm.so has no %s (built before the device-destination decode)" % name)
    return getattr(L, name)


def _device_header(buf, what):
    """(xyzct, KLB data type) of an in-memory .lfm, ValueError when it holds no header."""
    import struct
    if len(buf) < 43:
        raise ValueError("%s: %d bytes hold no .lfm header" % (what, len(buf)))
    head = bytes(memoryview(buf)[:43]) if not isinstance(buf, np.ndarray) else buf[:43].tobytes()
    dt = head[42]
    if dt not in _KLB_TORCH:
        raise ValueError("%s: unknown data type %d in the header" % (what, dt))
    return list(struct.unpack_from("<5I", head, 2)), dt


def _device_out(what, dt, shape, out, device):
    """The CUDA tensor a device-destination decode writes: `out` checked
    (contiguous, on a CUDA device, the file's dtype -- int16 stands in for
    uint16 as in Encoder._operand -- and the size), or a fresh one on `device`.
    A non-default current stream is synchronised: the library orders its
    writes after the null stream's work only."""
    if not _HAVE_TORCH:
        raise LfmError("%s needs PyTorch" % what)
    tdt = getattr(torch, _KLB_TORCH[dt])
    count = int(np.prod(shape))
    if out is None:
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("%s: device must be a CUDA device, not %s" % (what, device))
        out = torch.empty(tuple(shape), dtype=tdt, device=device)
    else:
        if not isinstance(out, torch.Tensor) or not out.is_cuda:
            raise ValueError("%s: out must be a torch CUDA tensor" % what)
        if not out.is_contiguous():
            raise ValueError("%s: out must be contiguous (got strides %s)" % (what, out.stride(),))
        if out.dtype != tdt and not (dt == 1 and out.dtype == torch.int16):
            raise ValueError("%s: the file holds %s, out is %s" % (what, tdt, out.dtype))
        if out.numel() != count:
            raise ValueError("%s: out holds %d elements, the result is %s" % (what, out.numel(), tuple(shape)))
        if device is not None and torch.device(device).index not in (None, out.device.index):
            raise ValueError("%s: out lives on %s, not on %s" % (what, out.device, device))
        out = out.view(tuple(shape))
    cur = torch.cuda.current_stream(out.device)
    if cur != torch.cuda.default_stream(out.device):
        cur.synchronize()
    return out


def decode_device(buf, out=None, device=None, num_threads=-1, return_stats=False):
    """Decode an in-memory .lfm into device memory (lfm_decode_memory_device):
    returns a torch CUDA tensor [t, c, z, y, x] in the file's dtype (uint16 for
    a KLB uint16 file), `out` itself (viewed in that shape) when given; with
    return_stats also the lfm_decode_stats as a dict.  The library's writes
    come after the null stream's work on the tensor's device; when the call
    returns, any stream may read the tensor.  After an LfmError the tensor's
    contents are unspecified."""
    fn = _need("lfm_decode_memory_device")
    xyzct, dt = _device_header(buf, "decode_device")
    out = _device_out("decode_device", dt, xyzct[::-1], out, device)
    st = DecodeStats()
    _check(fn(_addr(buf), len(buf), out.data_ptr(), out.numel() * out.element_size(), num_threads, ctypes.byref(st)),
           "lfm_decode_memory_device")
    return (out, st.as_dict()) if return_stats else out


def decode_roi_device(buf, lb, ub, out=None, device=None, num_threads=-1, return_stats=False):
    """Region lb .. ub (inclusive, [x, y, z, c, t]) of an in-memory .lfm into
    device memory (lfm_decode_memory_roi_device); as decode_device otherwise."""
    fn = _need("lfm_decode_memory_roi_device")
    xyzct, dt = _device_header(buf, "decode_roi_device")
    lb, ub = [int(v) for v in lb], [int(v) for v in ub]
    if len(lb) != 5 or len(ub) != 5 or any(u < l or l < 0 or u >= d for l, u, d in zip(lb, ub, xyzct)):
        raise ValueError("decode_roi_device: region %s .. %s lies outside the image %s" % (lb, ub, xyzct))
    shape = [u - l + 1 for l, u in zip(lb, ub)][::-1]
    out = _device_out("decode_roi_device", dt, shape, out, device)
    st = DecodeStats()
    _check(fn(_addr(buf), len(buf), _u32(lb), _u32(ub), out.data_ptr(), out.numel() * out.element_size(),
              num_threads, ctypes.byref(st)), "lfm_decode_memory_roi_device")
    return (out, st.as_dict()) if return_stats else out


def read_lfm_device(path, out=None, device=None, num_threads=-1, return_stats=False, family=None):
    """Read a .lfm file and decode it into device memory (decode_device)."""
    if family is not None:
        set_family(family)
    with open(path, "rb") as f:
        buf = f.read()
    return decode_device(buf, out=out, device=device, num_threads=num_threads, return_stats=return_stats)


# ------------------------------------------- streaming to and from a file --
class Writer:
    """lfm_writer: one .lfm file from block layers appended over time.

    shape: the stack's [t, c, z, y, x] (or fewer leading dims); its extent
    along the stream axis (t when t > 1, else c when c > 1, else z; `.axis`
    is the xyzct index) is the CAPACITY, the most that may be appended.  The
    other arguments are write_lfm's.  append() takes a numpy array or a CUDA
    tensor (not both in one writer) of `count` indices along the axis; close()
    finalises the file and returns the lfm_writer_stats dict.  The closed file
    is byte-identical to write_lfm of the appended stack.  Leaving a `with`
    block closes the writer, or aborts it (the file is removed) on an
    exception; a writer dropped without close() is aborted too.  A file that
    was never closed (the process died) is not a valid .lfm, but the writer
    checkpoints its table: recover() turns such a file into the .lfm of its
    complete layers, and Reader(path, live=True) reads them meanwhile."""

    def __init__(self, path, shape, dtype=np.uint16, predictor_request=0, nnum=13, video=0, block_size=None,
                 pixel_size=None, compression=1, metadata=None, device=-1, num_threads=-1):
        shape = [int(v) for v in shape]
        if not 1 <= len(shape) <= 5:
            raise ValueError("Writer: shape is [t, c, z, y, x] or fewer leading dims")
        shape = [1] * (5 - len(shape)) + shape
        self._xyzct = shape[::-1]
        self._dtype = np.dtype(dtype)
        if device < 0 and _HAVE_TORCH and torch.cuda.is_available():
            device = torch.cuda.current_device()
        self._device = device
        fn = _need("lfm_writer_open")
        h = ctypes.c_void_p()
        rc = fn(ctypes.byref(h), os.fsencode(path), _u32(self._xyzct), DTYPES[self._dtype],
                (int(predictor_request) & 0x7F) | ((1 if video else 0) << 7), int(nnum),
                _f32(pixel_size) if pixel_size is not None else None,
                _u32(block_size) if block_size is not None else None, compression, _meta(metadata), int(device),
                num_threads)
        _check(rc, "lfm_writer_open")
        self._h = h
        self.axis = int(lib().lfm_writer_axis(h))
        self._frame = shape[5 - self.axis:]  # the dims below the axis, [.., y, x]
        self.stats = None

    def _count(self, got):
        want = [d for d in self._frame if d != 1]
        got = [int(d) for d in got if d != 1]
        if got == want:
            return 1
        if got[1:] == want:
            return got[0]
        raise ValueError("Writer.append: shape %s is neither %s nor (count,) + that" % (list(got), self._frame))

    def append(self, a):
        """Append a's indices along the stream axis: a numpy array or CUDA
        tensor shaped like the stack below the axis, with an optional leading
        count.  The data may be reused when the call returns."""
        if self._h is None:
            raise LfmError("Writer.append: the writer is closed")
        if _HAVE_TORCH and isinstance(a, torch.Tensor) and a.is_cuda:
            kt = Encoder._TORCH_KLB.get(str(a.dtype))
            if kt != DTYPES[self._dtype] and not (DTYPES[self._dtype] == 1 and str(a.dtype) == "torch.int16"):
                raise LfmError("Writer.append: tensor dtype %s, the stack holds %s" % (a.dtype, self._dtype))
            if not a.is_contiguous():
                raise LfmError("device input must be contiguous (got strides %s)" % (a.stride(),))
            if self._device >= 0 and a.device.index != self._device:
                raise LfmError("device input lives on cuda:%d, the writer on cuda:%d" % (a.device.index, self._device))
            # (the library reads after the null stream's work: see Encoder._operand)
            cur = torch.cuda.current_stream(a.device)
            if cur != torch.cuda.default_stream(a.device):
                cur.synchronize()
            ptr, dev, shape = a.data_ptr(), 1, a.shape
        else:
            if _HAVE_TORCH and isinstance(a, torch.Tensor):
                a = a.numpy()
            a = np.ascontiguousarray(a)
            if a.dtype != self._dtype:
                raise LfmError("Writer.append: array dtype %s, the stack holds %s" % (a.dtype, self._dtype))
            ptr, dev, shape = a.ctypes.data, 0, a.shape
        count = self._count(shape)
        _check(lib().lfm_writer_append(self._h, ptr, dev, count), "lfm_writer_append")
        del a

    def flush(self, sync=False):
        """Wait until every whole layer appended so far is in the file, payload
        and table entries (lfm_writer_flush); sync=True also fdatasyncs.
        Returns the indices along the axis that recover() would now keep and a
        live Reader shows after refresh(); the part of a layer the writer
        holds back is not among them."""
        if self._h is None:
            raise LfmError("Writer.flush: the writer is closed")
        committed = ctypes.c_uint64()
        _check(_need("lfm_writer_flush")(self._h, 1 if sync else 0, ctypes.byref(committed)), "lfm_writer_flush")
        return int(committed.value)

    def close(self):
        """Finalise the file; returns the lfm_writer_stats dict (also `.stats`)."""
        if self._h is None:
            return self.stats
        h, self._h = self._h, None
        st = WriterStats()
        _check(lib().lfm_writer_close(h, ctypes.byref(st)), "lfm_writer_close")
        self.stats = st.as_dict()
        return self.stats

    def abort(self):
        """Drop the writer and remove the file."""
        if self._h is not None:
            h, self._h = self._h, None
            lib().lfm_writer_abort(h)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self.abort()
        return False

    def __del__(self):
        try:
            self.abort()
        except Exception:
            pass


class Reader:
    """lfm_reader: region reads of a .lfm file that fetch only the bytes of the
    blocks the region depends on (open reads the header and the offset table).
    .shape is [t, c, z, y, x]; .bytes_read counts every byte read from the
    file so far, header and table included.

    live=True (lfm_reader_open_live) also takes a file whose Writer has not
    closed it: .shape then shows the committed whole layers along the stream
    axis (0 before the first), refresh() picks up what the writer has
    checkpointed since (Writer.flush), and a region past the extent raises
    LfmError code 3.  After the writer's close, refresh() before reading on."""

    def __init__(self, path, live=False):
        name = "lfm_reader_open_live" if live else "lfm_reader_open"
        fn = _need(name)
        h = ctypes.c_void_p()
        self._h = None
        self._live = bool(live)
        _check(fn(ctypes.byref(h), os.fsencode(path)), name)
        self._h = h
        self._info()

    def _info(self):
        h = self._h
        xyzct, bs = (ctypes.c_uint32 * 5)(), (ctypes.c_uint32 * 5)()
        dt, hv, nn, fb = ctypes.c_int(), ctypes.c_uint8(), ctypes.c_uint8(), ctypes.c_uint64()
        _check(lib().lfm_reader_info(h, xyzct, ctypes.byref(dt), bs, ctypes.byref(hv), ctypes.byref(nn),
                                     ctypes.byref(fb)), "lfm_reader_info")
        self._xyzct = list(xyzct)
        self._dt = dt.value
        self.shape = tuple(self._xyzct[::-1])
        self.dtype = np.dtype(NP_OF[dt.value])
        self.block_size = list(bs)
        self.header_version = hv.value
        self.nnum = nn.value
        self.file_bytes = fb.value

    def refresh(self):
        """Look at the file again (lfm_reader_refresh): a live reader takes up
        the layers the writer has committed since, or the closed file when the
        writer has closed it meanwhile.  Returns the shape, as `.shape` now is."""
        if self._h is None:
            raise LfmError("Reader.refresh: the reader is closed")
        extent = ctypes.c_uint32()
        _check(_need("lfm_reader_refresh")(self._h, ctypes.byref(extent)), "lfm_reader_refresh")
        self._info()
        return self.shape

    @property
    def bytes_read(self):
        return int(lib().lfm_reader_bytes_read(self._h)) if self._h else 0

    def read(self, lb, ub, device=None, out=None, return_stats=False, num_threads=-1):
        """Region lb .. ub (inclusive, [x, y, z, c, t]) as an array [t, c, z, y, x]
        of the region: numpy, or a torch CUDA tensor when `device` or a CUDA
        tensor `out` is given (as decode_roi / decode_roi_device otherwise)."""
        if self._h is None:
            raise LfmError("Reader.read: the reader is closed")
        lb, ub = [int(v) for v in lb], [int(v) for v in ub]
        # (a live reader's extent is the library's to judge: a region past it is its code 3)
        if len(lb) != 5 or len(ub) != 5 or any(u < l or l < 0 or (u >= d and not self._live)
                                               for l, u, d in zip(lb, ub, self._xyzct)):
            raise ValueError("Reader.read: region %s .. %s lies outside the image %s" % (lb, ub, self._xyzct))
        shape = [u - l + 1 for l, u in zip(lb, ub)][::-1]
        st = DecodeStats()
        to_device = device is not None or (_HAVE_TORCH and isinstance(out, torch.Tensor))
        if to_device:
            out = _device_out("Reader.read", self._dt, shape, out, device)
            ptr, nbytes = out.data_ptr(), out.numel() * out.element_size()
        else:
            if out is None:
                out = np.empty(shape, dtype=self.dtype)
            else:
                if not isinstance(out, np.ndarray) or not out.flags.c_contiguous or not out.flags.writeable:
                    raise ValueError("Reader.read: out must be a writeable C-contiguous numpy array")
                if out.dtype != self.dtype or out.size != int(np.prod(shape)):
                    raise ValueError("Reader.read: out holds %d x %s, the region is %s x %s"
                                     % (out.size, out.dtype, shape, self.dtype))
                out = out.reshape(shape)
            ptr, nbytes = out.ctypes.data, out.nbytes
        _check(lib().lfm_reader_read(self._h, _u32(lb), _u32(ub), ptr, nbytes, 1 if to_device else 0, num_threads,
                                     ctypes.byref(st)), "lfm_reader_read")
        return (out, st.as_dict()) if return_stats else out

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            lib().lfm_reader_close(h)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def recover(path, out=None, verify=True, num_threads=-1):
    """Turn a file its Writer never closed into the .lfm of its complete layers
    (lfm_recover): in place when `out` is None -- not atomic, an interrupted
    in-place recovery can leave the file beyond repair -- else `path` is only
    read and the result written to `out`.  verify=True decodes every stream of
    the committed layers (bzip2 CRCs and lengths; on the GPU when one is
    visible) and keeps the longest prefix of layers that pass; verify=False
    trusts the table, which is only safe after a process crash.  Returns the
    lfm_recover_stats dict (`kept` indices along the axis; `already_valid` for
    a closed file, which is left alone); LfmError code 3 when no complete
    layer survives."""
    st = RecoverStats()
    _check(_need("lfm_recover")(os.fsencode(path), os.fsencode(out) if out is not None else None,
                                1 if verify else 0, num_threads, ctypes.byref(st)), "lfm_recover")
    return st.as_dict()


# ------------------------------------------------------- multi-GPU reader --
def set_decode_devices(devices=None):
    """Devices the whole-image readers farm block-layer ranges to
    (lfm_set_decode_devices; a device may repeat); None or [] restores the
    default: env LFM_DECODE_GPUS, empty without it.  Fewer than two entries:
    every reader runs on the current device as ever."""
    devices = list(devices or [])
    arr = (ctypes.c_int * max(1, len(devices)))(*devices)
    _check(_need("lfm_set_decode_devices")(arr, len(devices)), "lfm_set_decode_devices")


def get_decode_devices():
    arr = (ctypes.c_int * 256)()
    n = _need("lfm_get_decode_devices")(arr, 256)
    return list(arr[:min(n, 256)])


def default_decode_devices(n_visible):
    """env LFM_DECODE_GPUS parsed for n_visible devices (no device call)."""
    arr = (ctypes.c_int * 256)()
    n = _need("lfm_default_decode_devices")(int(n_visible), arr, 256)
    return list(arr[:min(n, 256)])


def release_decoders():
    """End the readers' kept workers; their device / pinned buffers are freed."""
    _need("lfm_release_decoders")()


def decode_shard_plan(buf, n):
    """(axis, [(first, count), ...]) of lfm_decode_shard_plan: how the file is
    cut for n workers, along xyzct index `axis`."""
    fn = _need("lfm_decode_shard_plan")
    axis = ctypes.c_int()
    cap = max(1, int(n))
    first, count = (ctypes.c_uint32 * cap)(), (ctypes.c_uint32 * cap)()
    s = fn(_addr(buf), len(buf), int(n), ctypes.byref(axis), first, count, cap)
    if s <= 0:
        raise LfmError("lfm_decode_shard_plan: the buffer holds no .lfm header")
    return axis.value, [(first[w], count[w]) for w in range(min(s, cap))]


def _multi_stats(st, shards, n):
    d = st.as_dict()
    d["shards"] = [shards[w].as_dict() for w in range(min(max(st.workers, 0), n))]
    return d


def decode_multi(buf, num_threads=-1, return_stats=False):
    """lfm_decode_memory_multi: decode an in-memory .lfm into a numpy array
    [t, c, z, y, x] with one worker per entry of the decode device list
    (set_decode_devices); with return_stats also the lfm_decode_multi_stats as
    a dict, its "shards" the list of lfm_decode_shard dicts."""
    fn = _need("lfm_decode_memory_multi")
    xyzct, dt = _device_header(buf, "decode_multi")
    out = np.empty(tuple(xyzct[::-1]), dtype=NP_OF[dt])
    st = DecodeMultiStats()
    cap = max(1, len(get_decode_devices()))
    shards = (DecodeShard * cap)()
    _check(fn(_addr(buf), len(buf), out.ctypes.data, num_threads, ctypes.byref(st), shards, cap),
           "lfm_decode_memory_multi")
    return (out, _multi_stats(st, shards, cap)) if return_stats else out


def decode_device_sharded(buf, devices=None, outs=None, return_stats=False):
    """lfm_decode_memory_multi_device: decode an in-memory .lfm into one torch
    CUDA tensor per shard, each on its own device, side by side.  devices: one
    CUDA device per worker (default: the decode device list, else the current
    device); the file is cut as decode_shard_plan(buf, len(devices)) says and
    shard w lands on devices[w].  outs: the tensors to decode into instead,
    one per shard of decode_shard_plan(buf, len(outs)), each the shard's size.
    Returns (axis, [(first, tensor), ...]), the tensors shaped [t, c, z, y, x]
    with the shard's extent along xyzct index `axis`; with return_stats also
    the stats dict of decode_multi.  Ordering per tensor as decode_device."""
    fn = _need("lfm_decode_memory_multi_device")
    xyzct, dt = _device_header(buf, "decode_device_sharded")
    if not _HAVE_TORCH:
        raise LfmError("decode_device_sharded needs PyTorch")
    if outs is not None:
        n = len(outs)
    else:
        if devices is None:
            devices = get_decode_devices() or [torch.cuda.current_device()]
        devices = [torch.device("cuda", d) if isinstance(d, int) else torch.device(d) for d in devices]
        n = len(devices)
    if n < 1:
        raise ValueError("decode_device_sharded: no destination")
    axis, plan = decode_shard_plan(buf, n)
    if outs is not None and len(plan) != n:
        raise ValueError("decode_device_sharded: %d tensors, but %d workers get %d shards" % (n, n, len(plan)))
    tensors = []
    for w, (first, count) in enumerate(plan):
        shape = xyzct[::-1]
        shape[4 - axis] = count
        tensors.append(_device_out("decode_device_sharded", dt, shape, None if outs is None else outs[w],
                                   None if outs is not None else devices[w]))
    S = len(tensors)
    ptrs = (ctypes.c_void_p * S)(*[t.data_ptr() for t in tensors])
    sizes = (ctypes.c_uint64 * S)(*[t.numel() * t.element_size() for t in tensors])
    st = DecodeMultiStats()
    shards = (DecodeShard * S)()
    _check(fn(_addr(buf), len(buf), ptrs, sizes, S, -1, ctypes.byref(st), shards, S),
           "lfm_decode_memory_multi_device")
    res = (axis, [(first, t) for (first, _), t in zip(plan, tensors)])
    return res + (_multi_stats(st, shards, S),) if return_stats else res


# ------------------------------------------------------ device primitives --
def _stream(stream):
    if stream is None:
        return None
    return ctypes.c_void_p(int(stream.cuda_stream) if hasattr(stream, "cuda_stream") else int(stream))


def crop_device(d_src, src_dims, lb, n, bpp, d_dst, stream=None):
    """lfm_hip_crop_region: the box lb .. lb + n - 1 ([x, y, z, c, t]) of a device
    image of src_dims (bpp bytes per sample) into the dense device array d_dst
    (tensors or raw pointers); asynchronous on `stream`."""
    fn = _need("lfm_hip_crop_region")
    p = lambda t: t.data_ptr() if hasattr(t, "data_ptr") else int(t)  # noqa: E731
    if len(src_dims) != 5 or len(lb) != 5 or len(n) != 5:
        raise ValueError("crop_device: src_dims, lb and n have five entries")
    if any(int(v) < 0 or int(v) >= 1 << 32 for v in list(src_dims) + list(lb) + list(n)):
        raise ValueError("crop_device: extents are 32-bit unsigned")
    _check(fn(p(d_src), _u32(src_dims), _u32(lb), _u32(n), int(bpp), p(d_dst), _stream(stream)),
           "lfm_hip_crop_region")


def scatter_blocks_device(d_blocks, stride, first, count, dims, bs, bpp, d_img, stream=None):
    """lfm_hip_scatter_blocks: blocks first .. first + count - 1 of the x-fastest
    block grid (dims, bs: [x, y, z, c, t]; bpp bytes per sample), block first + i
    at d_blocks + i * stride with its bytes x fastest, then y, z, c, t, into the
    device image d_img (tensors or raw pointers); asynchronous on `stream`.
    The block range, the stride and the extents are checked here: the library
    launches whatever it is given."""
    fn = _need("lfm_hip_scatter_blocks")
    p = lambda t: t.data_ptr() if hasattr(t, "data_ptr") else int(t)  # noqa: E731
    if len(dims) != 5 or len(bs) != 5:
        raise ValueError("scatter_blocks_device: dims and bs have five entries")
    if any(int(v) < 1 or int(v) >= 1 << 32 for v in list(dims) + list(bs) + [bpp]):
        raise ValueError("scatter_blocks_device: extents are 32-bit unsigned and not 0")
    total = int(np.prod([-(-int(d) // int(b)) for d, b in zip(dims, bs)], dtype=np.uint64))
    if int(first) < 0 or int(count) < 1 or int(first) + int(count) > total:
        raise ValueError("scatter_blocks_device: blocks %d .. %d of a grid of %d"
                         % (first, int(first) + int(count) - 1, total))
    block_bytes = int(np.prod([min(int(d), int(b)) for d, b in zip(dims, bs)], dtype=np.uint64)) * int(bpp)
    if not block_bytes <= int(stride) < 1 << 32:
        raise ValueError("scatter_blocks_device: stride %d, a block holds up to %d bytes" % (stride, block_bytes))
    _check(fn(p(d_blocks), int(stride), int(first), int(count), _u32(dims), _u32(bs), int(bpp), p(d_img),
              _stream(stream)), "lfm_hip_scatter_blocks")


def predict_device(d_in, d_out, W, H, nframes, T, family, predictor, video=0, z0=0, d_prev=None, stream=None):
    """Launch the fused predictor + symbolize kernel on device tensors (or raw pointers)."""
    p = lambda t: None if t is None else (t.data_ptr() if hasattr(t, "data_ptr") else int(t))  # noqa: E731
    rc = lib().lfm_hip_predict(p(d_in), p(d_prev), p(d_out), W, H, nframes, T, FAMILIES.get(family, family),
                               predictor, video, z0, _stream(stream))
    _check(rc, "lfm_hip_predict")


def unpredict_device(d_sym, d_out, W, H, nframes, T, family, predictor, video=0, z0=0, d_prev=None, stream=None):
    """Inverse predictor (decode) on device tensors: symbols -> pixels."""
    p = lambda t: None if t is None else (t.data_ptr() if hasattr(t, "data_ptr") else int(t))  # noqa: E731
    rc = lib().lfm_hip_unpredict(p(d_sym), p(d_prev), p(d_out), W, H, nframes, T, FAMILIES.get(family, family),
                                 predictor, video, z0, _stream(stream))
    _check(rc, "lfm_hip_unpredict")


def unpredict_device_async(d_sym, d_out, W, H, nframes, T, family, predictor, video=0, z0=0, d_prev=None, status=None,
                           stream=None):
    """lfm_hip_unpredict_async: unpredict_device without the synchronisation.  The
    kernels are queued on `stream` and the call's status word is copied behind
    them into status[0] (`status`: a pinned int32 host tensor); once the stream
    has passed that point the word goes to unpredict_check."""
    if status is None or not status.is_pinned() or str(status.dtype) != "torch.int32" or status.numel() < 1:
        raise ValueError("unpredict_device_async: status is a pinned int32 host tensor")
    p = lambda t: None if t is None else (t.data_ptr() if hasattr(t, "data_ptr") else int(t))  # noqa: E731
    rc = lib().lfm_hip_unpredict_async(p(d_sym), p(d_prev), p(d_out), W, H, nframes, T, FAMILIES.get(family, family),
                                       predictor, video, z0, status.data_ptr(), _stream(stream))
    _check(rc, "lfm_hip_unpredict_async")


def unpredict_check(status):
    """lfm_hip_unpredict_check on a status word of unpredict_device_async (the
    tensor or its value): returns when the pixels are valid, a repaired band
    hand-over timeout included (reported on stderr); raises otherwise."""
    word = int(status.reshape(-1)[0]) if hasattr(status, "reshape") else int(status)
    _check(lib().lfm_hip_unpredict_check(word), "lfm_hip_unpredict_check")


UNPREDICT_PATHS = ("chain", "frame-wave", "one-wave")


def unpredict_path(W, H, T):
    """Which inverse-predictor kernel decodes W x H frames of lenslet size T: an
    index into UNPREDICT_PATHS, or -1 for a shape the inverse rejects.  No GPU."""
    return int(lib().lfm_hip_unpredict_path(W, H, T))


PREDICT_KERNELS = ("copy", "generic", "ring", "vec", "vec_pair", "cands")
PREDICT_MAX_LAUNCHES = 7


def predict_plan(W, H, nframes, T, family, predictor, video=0, z0=0, candidates=False, aligned=True):
    """lfm_hip_predict_plan: the launches predict_device (or, with `candidates`,
    predict_candidates_device) makes for these arguments, in order, as dicts of
    the lfm_predict_launch fields with the kernel's name from PREDICT_KERNELS.
    `aligned`: the call's pointers are 16-byte aligned.  Launches nothing; no
    GPU is needed once predict_set_pieces has forced a piece count."""
    out = (PredictLaunch * PREDICT_MAX_LAUNCHES)()
    n = lib().lfm_hip_predict_plan(W, H, nframes, T, FAMILIES.get(family, family), predictor, int(video), z0,
                                   int(bool(candidates)), int(bool(aligned)), out, PREDICT_MAX_LAUNCHES)
    if n < 0:
        raise LfmError("lfm_hip_predict_plan refused %r" % ((W, H, nframes, T, family, predictor, video, z0),))
    plans = []
    for i in range(n):
        d = {f: getattr(out[i], f) for f, _ in PredictLaunch._fields_}
        d["kernel"] = PREDICT_KERNELS[d["kernel"]]
        plans.append(d)
    return plans


def predict_set_pieces(n):
    """lfm_hip_predict_set_pieces, a test hook: force the forward predictor's
    row-piece count for the whole process (0 = automatic); returns the
    previous value."""
    return int(lib().lfm_hip_predict_set_pieces(int(n)))


def predict_candidates_device(d_frame, d_out7, W, H, T, family, stream=None):
    """The seven spatial candidates of one frame in one launch (d_out7: 7*H*W uint16)."""
    rc = lib().lfm_hip_predict_candidates(d_frame.data_ptr(), d_out7.data_ptr(), W, H, T,
                                          FAMILIES.get(family, family), _stream(stream))
    _check(rc, "lfm_hip_predict_candidates")


def select_device(d_frame, W, H, T, family, stream=None):
    ent = (ctypes.c_float * 8)()
    k = ctypes.c_int()
    rc = lib().lfm_hip_select(d_frame.data_ptr(), W, H, T, FAMILIES.get(family, family), ent, ctypes.byref(k), None,
                              _stream(stream))
    _check(rc, "lfm_hip_select")
    return k.value, np.array(list(ent), dtype=np.float32)


def entropy_device(d_cand, npix=None, stream=None):
    e = ctypes.c_float()
    n = d_cand.numel() if npix is None else npix
    _check(lib().lfm_hip_entropy2d(d_cand.data_ptr(), n, ctypes.byref(e), _stream(stream)), "lfm_hip_entropy2d")
    return e.value


def entropy_hist_device(d_cands, npix, stream=None):
    """lfm_hip_entropy2d_hist: the integer bigram histograms the selection
    kernels count for a list of 1..8 int16 device tensors (views at any 2-byte
    offset) of at least npix symbols each, as a (ncand, nchunks, 65536) uint32
    array, bin = (val << 8) | partner."""
    ncand, nchunks = len(d_cands), -(-int(npix) // 450000)
    if not 1 <= ncand <= 8 or npix < 1 or any(str(t.dtype) != "torch.int16" or t.numel() < npix or
                                              not t.is_contiguous() for t in d_cands):
        raise ValueError("entropy_hist_device: 1..8 contiguous int16 tensors of npix >= 1 symbols each")
    ptrs = (ctypes.c_void_p * ncand)(*[t.data_ptr() for t in d_cands])
    d_hist = torch.empty((ncand, nchunks, 65536), dtype=torch.int32, device=d_cands[0].device)
    _check(lib().lfm_hip_entropy2d_hist(ptrs, ncand, npix, d_hist.data_ptr(), _stream(stream)),
           "lfm_hip_entropy2d_hist")
    return d_hist.cpu().numpy().view(np.uint32)


def set_bzip2_multiblock(on):
    """GPU bzip2 of streams of several bzip2 blocks on (default) or off (such
    streams go to the host library); returns the previous setting."""
    return bool(lib().lfm_set_bzip2_multiblock(1 if on else 0))


def get_bzip2_multiblock():
    return bool(lib().lfm_get_bzip2_multiblock())


def bzip2_device(d_img, dims, block, bpp, level=None, first=0, count=None, stream=None, multi=False):
    """GPU bzip2 of the x-fastest block grid of a device image (torch tensor
    holding dims[4]*...*dims[0]*bpp bytes).  Returns ([bytes or None per
    stream], flags): None where the stream was handed to the host library.
    multi=True: lfm_hip_bzip2_blocks_multi, which also compresses the streams
    libbzip2 cuts into several bzip2 blocks."""
    nb = [-(-d // b) for d, b in zip(dims, block)]
    total = int(np.prod(nb))
    count = total - first if count is None else count
    block_bytes = int(np.prod(block)) * bpp
    level = min(9, -(-block_bytes // 100000)) if level is None else level
    if multi:
        ws_bytes = lib().lfm_hip_bzip2_workspace_bytes_multi(count, block_bytes, level)
    else:
        ws_bytes = lib().lfm_hip_bzip2_workspace_bytes(count, block_bytes)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=d_img.device)
    out_cap = lib().lfm_hip_bzip2_out_cap(block_bytes)
    pay = torch.empty(count * out_cap, dtype=torch.uint8, device=d_img.device)
    sizes = (ctypes.c_uint64 * count)()
    flags = (ctypes.c_uint32 * count)()
    fn = lib().lfm_hip_bzip2_blocks_multi if multi else lib().lfm_hip_bzip2_blocks
    _check(fn(d_img.data_ptr(), _u32(dims), _u32(block), bpp, first, count, level,
              ws.data_ptr(), ws_bytes, pay.data_ptr(), sizes, flags, _stream(stream)),
           "lfm_hip_bzip2_blocks_multi" if multi else "lfm_hip_bzip2_blocks")
    host = pay[:int(sum(sizes))].cpu().numpy().tobytes()
    out, o = [], 0
    for i in range(count):
        if flags[i]:
            out.append(None)
        else:
            out.append(host[o:o + sizes[i]])
            o += sizes[i]
    return out, list(flags)


BWT_STATS = ("chunks_tiny", "chunks_small", "chunks_big", "chunks_segmented", "first_ties", "left_runs",
             "text_rounds", "restarted", "rank_form", "doubling_rounds", "flag_periodic")


def bzip2_last_bwt_stats():
    """The path the BWT sort of this thread's last bzip2_device call took
    (lfm_hip_bzip2_last_bwt_stats, lfm_hip.h), as a dict over BWT_STATS."""
    out = (ctypes.c_uint32 * 12)()
    lib().lfm_hip_bzip2_last_bwt_stats(out)
    return dict(zip(BWT_STATS, list(out)))


SORT_JOB_CAPS = (512, 1024, 2048, 4096)


def bzip2_last_sort_jobs():
    """The sort jobs of this thread's last bzip2_device call per sorter
    capacity (lfm_hip_bzip2_last_sort_jobs, lfm_hip.h), as a dict over
    SORT_JOB_CAPS."""
    out = (ctypes.c_uint32 * 4)()
    lib().lfm_hip_bzip2_last_sort_jobs(out)
    return dict(zip(SORT_JOB_CAPS, list(out)))


def bzip2_last_place_path():
    """How the sorted rotations of this thread's last bzip2_device call were
    placed (lfm_hip_bzip2_last_place_path, lfm_hip.h): 0 not at all (restart),
    1 by the chunk sorts, 2 by the placement kernel over the whole batch."""
    return int(lib().lfm_hip_bzip2_last_place_path())


def set_bunzip2_multiblock(on):
    """GPU decode of streams of several bzip2 blocks on (default) or off (such
    streams are decoded by the host library); returns the previous setting."""
    return bool(lib().lfm_set_bunzip2_multiblock(1 if on else 0))


def get_bunzip2_multiblock():
    return bool(lib().lfm_get_bunzip2_multiblock())


def set_bunzip2_periodic(on):
    """GPU decode of bzip2 blocks with an exactly periodic text on, or off (the
    default: their streams are decoded by the host library); returns the
    previous setting.  Applies to bunzip2_device and to every reader."""
    return bool(lib().lfm_set_bunzip2_periodic(1 if on else 0))


def get_bunzip2_periodic():
    return bool(lib().lfm_get_bunzip2_periodic())


def bunzip2_max_parts(out_stride, level):
    """bzip2 blocks a stream of at most out_stride decoded bytes can hold at
    `level`: the slots it owns in bunzip2_device(..., multi=True).  0 for a
    level outside 1..9.  No GPU."""
    return int(lib().lfm_hip_bunzip2_max_parts(out_stride, level))


def bunzip2_device(streams, out_stride, device="cuda", stream=None, multi=False, level=None):
    """GPU bzip2 decode of streams (bytes objects).  Returns ([bytes per
    stream, or None where the device flagged it for the host library],
    flags): flag 1 = host library, 2 = block CRC mismatch.
    multi=False: lfm_hip_bunzip2_blocks, single-block streams only.
    multi=True: lfm_hip_bunzip2_blocks_multi, which also decodes streams of up
    to bunzip2_max_parts(out_stride, level) bzip2 blocks of `level` (default:
    the writer's, min(9, ceil(out_stride / 100000)))."""
    count = len(streams)
    offs = np.zeros(count + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in streams])
    blob = b"".join(streams) + bytes(64)
    d_pay = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(device)
    level = max(1, min(9, -(-out_stride // 100000))) if level is None else level
    if multi:
        ws_bytes = lib().lfm_hip_bunzip2_workspace_bytes_multi(count, out_stride, level)
    else:
        ws_bytes = lib().lfm_hip_bunzip2_workspace_bytes(count, out_stride)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    out = torch.empty(count * out_stride, dtype=torch.uint8, device=device)
    lens = (ctypes.c_uint32 * count)()
    flags = (ctypes.c_uint32 * count)()
    p_offs = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    if multi:
        _check(lib().lfm_hip_bunzip2_blocks_multi(d_pay.data_ptr(), p_offs, count, out.data_ptr(), out_stride, level,
                                                  ws.data_ptr(), ws_bytes, lens, flags, _stream(stream)),
               "lfm_hip_bunzip2_blocks_multi")
    else:
        _check(lib().lfm_hip_bunzip2_blocks(d_pay.data_ptr(), p_offs, count, out.data_ptr(), out_stride,
                                            ws.data_ptr(), ws_bytes, lens, flags, _stream(stream)),
               "lfm_hip_bunzip2_blocks")
    host = out.cpu().numpy()
    res = [None if flags[i] else host[i * out_stride:i * out_stride + lens[i]].tobytes() for i in range(count)]
    return res, list(flags)


def synth_device(d_out, X, Y, Z, T, t_index=0, idx0=None, seed=0x4C464D00, z0=0, stream=None):
    """SURVEY 8(d) generator on the device: frames z0 .. z0+Z-1 of volume
    (0, t_index); idx0 defaults to z0*X*Y (a z-slab of a c = t = 1 stack,
    equal to oracle.synthetic_lf(..., z0=z0))."""
    if idx0 is None:
        idx0 = z0 * X * Y
    _check(lib().lfm_hip_synth(d_out.data_ptr(), X, Y, Z, T, t_index, z0, idx0, seed, _stream(stream)),
           "lfm_hip_synth")
