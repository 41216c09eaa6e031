"""ctypes view of the C ABI in include/crsdr.h (libcrsdr.so).

This is plumbing for tests and bench.py; the product boundary is the C ABI itself.  There is
no fallback: if the HIP extension is missing or no device is present, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("CRSDR_LIB") or os.path.join(_HERE, "libcrsdr.so")   # CRSDR_LIB: A/B a second build (diagnostics)
ROOT = os.path.dirname(_HERE)

MODE_FAITHFUL, MODE_DIGITAL = 0, 1
MEM_HOST, MEM_DEVICE = 0, 1
REFNOISE_ENABLED, OFFSET_BINARY, INPUT_READY, NO_LAG = 1, 2, 4, 8

# every symbol include/crsdr.h declares (tests check the .so exports all of them)
ABI_SYMBOLS = [
    "crsdr_abi_version", "crsdr_last_error", "crsdr_device_count",
    "crsdr_convtosigned", "crsdr_convtofloat", "crsdr_scalarmul", "crsdr_convto8bit",
    "crsdr_conj_dotproduct", "crsdr_magsquared", "crsdr_conjugatemul", "crsdr_indexofmax", "crsdr_fft",
    "crsdr_plan_create", "crsdr_plan_destroy", "crsdr_plan_reset", "crsdr_plan_set_stream",
    "crsdr_plan_submit", "crsdr_plan_fetch", "crsdr_plan_sync", "crsdr_plan_packet_bytes",
    "crsdr_plan_matrix_offset", "crsdr_plan_device_buffers", "crsdr_plan_bind_packet",
    "crsdr_plan_last_elapsed_ms", "crsdr_plan_enable_profiling", "crsdr_plan_kernel_times",
    "crsdr_plan_submit_batch", "crsdr_plan_fetch_block", "crsdr_plan_packet_stride", "crsdr_covariance",
    "crsdr_noisesubspace", "crsdr_pmusic2d", "crsdr_plan_bind_slab", "crsdr_assemble_slabs",
    "crsdr_device_info", "crsdr_host_alloc", "crsdr_host_free",
    "crsdr_plan_bind_slab_ex", "crsdr_exchange_geometry", "crsdr_exchange_rooted_blocks", "crsdr_assemble_slots",
    "crsdr_plan_set_frac_apply", "crsdr_plan_fetch_batch_async", "crsdr_plan_fetch_wait", "crsdr_exchange_unique_id", "crsdr_exchange_create", "crsdr_exchange_destroy", "crsdr_exchange_batch", "crsdr_exchange_schedule",
    "crsdr_exchange_bind_plan", "crsdr_exchange_submit_batch", "crsdr_exchange_fetch_rooted",
    "crsdr_doa_create", "crsdr_doa_destroy", "crsdr_doa_submit", "crsdr_doa_submit_plan", "crsdr_doa_fetch",
    "crsdr_doa_device_buffers", "crsdr_doa_last_submit", "crsdr_doa_set_peaks", "crsdr_doa_fetch_directions",
    "crsdr_doa_direction_buffers",
    "crsdr_beamform", "crsdr_doa_set_beams", "crsdr_doa_fetch_beams", "crsdr_doa_beam_buffers", "crsdr_doa_fetch_subspace",
    "crsdr_doa_set_smoothing", "crsdr_doa_fetch_smoothed", "crsdr_doa_set_order", "crsdr_doa_fetch_order", "crsdr_doa_order_buffers",
    "crsdr_smooth_covariance", "crsdr_source_order",
    "crsdr_doa_set_subbands", "crsdr_doa_fetch_subbands", "crsdr_doa_subband_buffers", "crsdr_subband_covariance",
    "crsdr_doa_set_subband_beams", "crsdr_doa_fetch_subband_beams", "crsdr_doa_subband_beam_buffers", "crsdr_subband_beamform",
    "crsdr_doa_set_spectrum", "crsdr_spectrum2d",
    "crsdr_doa_set_refine", "crsdr_doa_fetch_refined", "crsdr_doa_refined_buffers", "crsdr_refine2d",
    "crsdr_doa_set_esprit", "crsdr_doa_fetch_esprit", "crsdr_doa_esprit_buffers", "crsdr_esprit2d",
    "crsdr_doa_set_augment", "crsdr_doa_fetch_augmented", "crsdr_doa_augment_buffers", "crsdr_augment_covariance", "crsdr_augment_lags",
    "crsdr_plan_set_refcancel", "crsdr_plan_fetch_refcancel", "crsdr_plan_refcancel_buffers", "crsdr_refcancel",
    "crsdr_spectra_create", "crsdr_spectra_destroy", "crsdr_spectra_submit", "crsdr_spectra_submit_plan", "crsdr_spectra_fetch",
    "crsdr_spectra_device_buffers", "crsdr_spectra_last_submit", "crsdr_welch",
    "crsdr_caf_create", "crsdr_caf_destroy", "crsdr_caf_submit", "crsdr_caf_submit_plan", "crsdr_caf_fetch",
    "crsdr_caf_device_buffers", "crsdr_caf_last_submit", "crsdr_ambiguity",
    "crsdr_caf_set_cfar", "crsdr_caf_fetch_cfar", "crsdr_caf_cfar_device_buffers", "crsdr_cfar", "crsdr_cfar_alpha",
    "crsdr_caf_set_cfar_estimator", "crsdr_cfar_est", "crsdr_cfar_alpha_est",
    "crsdr_caf_set_cancel", "crsdr_caf_fetch_cancel", "crsdr_caf_cancel_device_buffers", "crsdr_ambiguity_cancel",
    "crsdr_caf_set_bearing", "crsdr_caf_fetch_bearing", "crsdr_caf_bearing_device_buffers", "crsdr_bearing",
    "crsdr_caf_set_beams", "crsdr_caf_fetch_beams", "crsdr_caf_beams_device_buffers", "crsdr_beam_maps", "crsdr_beam_fuse", "crsdr_caf_beam_steer",
    "crsdr_caf_set_beam_adapt", "crsdr_caf_fetch_beam_adapt", "crsdr_caf_beam_adapt_device_buffers", "crsdr_beam_adapt",
    "crsdr_caf_set_track", "crsdr_caf_track_reset", "crsdr_caf_fetch_track", "crsdr_caf_track_device_buffers", "crsdr_track_state_bytes", "crsdr_track",
    "crsdr_caf_set_integrate", "crsdr_caf_integrate_reset", "crsdr_caf_fetch_integrate", "crsdr_caf_integrate_device_buffers",
    "crsdr_map_integrate_state_bytes", "crsdr_map_integrate",
    "crsdr_caf_set_clean", "crsdr_caf_fetch_clean", "crsdr_caf_clean_device_buffers", "crsdr_ambiguity_clean",
]
CLEAN_SINGULAR, CLEAN_TARGET = 1, 2                             # tinfo[..., 1]: the first stage is singular; a target column's pivot failed
CLEAN_LAUNCHES = 9                                              # what a submit issues more with the cleaning on
INTEGRATE_ARRAY, INTEGRATE_BEAMS = 1, 2
TRACK_SRC_ARRAY, TRACK_SRC_FUSED = 0, 1
TRACK_FREE, TRACK_TENTATIVE, TRACK_CONFIRMED, TRACK_ENDED = 0, 1, 2, 3      # trk[..., 1]
BEARING_CONVENTIONAL, BEARING_ADAPTIVE = 1, 2
BEARING_KEEP_SPECTRUM = 1
BEARING_ZERO, BEARING_IDENTITY, BEARING_CELL = 1, 2, 4        # status bits 0, 1, 2: all-zero snapshot; W = I; a cell outside the map
REFCANCEL_SINGULAR, REFCANCEL_IDLE = 1, 2                     # status bit 0: the solve failed (g = 0); 2: the pass did not run
REFCANCEL_MAX_TAPS = 9
ESPRIT_OFF, ESPRIT_BESIDE, ESPRIT_ONLY = 0, 1, 2
ESPRIT_STATUS_ITERATIONS, ESPRIT_STATUS_PIVOT = 1, 2          # status bits 0 and 1
ESPRIT_FLAG_BETA, ESPRIT_FLAG_ALPHA = 1, 2                    # flag bits 0 and 1: cos(beta), cos(alpha) clamped
ESPRIT_MAX_K = 16
DOA_KEEP_SPECTRUM, DOA_KEEP_RXX = 1, 2
BEAM_OFF, BEAM_CONVENTIONAL, BEAM_MVDR = 0, 1, 2
SMOOTH_FB = 1
ORDER_OFF, ORDER_MDL, ORDER_AIC = 0, 1, 2
SPECTRUM_MUSIC, SPECTRUM_BARTLETT, SPECTRUM_CAPON = 0, 1, 2
WINDOW_RECT, WINDOW_HANN = 0, 1
XCHG_STAGED, XCHG_INPLACE = 0, 1
EXCHANGE_ID_BYTES = 128
KERNEL_REF_SPECTRUM, KERNEL_XCORR_LAG, KERNEL_PHASE_DOT, KERNEL_ALIGN_QUANT = 0, 1, 2, 3


class CrsdrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"crsdr error {code}: {msg}")
        self.code = code


def build(force: bool = False) -> str:
    """Compile libcrsdr.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    deps = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(ROOT, "include", "crsdr.h")]
    stale = force or not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps)
    if stale:
        subprocess.run(["make", "-C", csrc], check=True)
    return _SO


class XOp(C.Structure):
    """crsdr_xop: one point-to-point operation of an exchange batch (crsdr_exchange_schedule)."""
    _fields_ = [("peer", C.c_int32), ("is_recv", C.c_int32), ("buffer", C.c_int32), ("block", C.c_int32),
                ("offset", C.c_uint64), ("bytes", C.c_uint64)]


class PlanDesc(C.Structure):
    _fields_ = [("nrows", C.c_int32), ("blocksize", C.c_int32), ("mode", C.c_int32), ("device", C.c_int32),
                ("row_begin", C.c_int32), ("row_count", C.c_int32), ("max_batch", C.c_int32), ("reserved", C.c_uint32)]


class DoaDesc(C.Structure):
    _fields_ = [("nrows", C.c_int32), ("blocksize", C.c_int32), ("device", C.c_int32), ("max_batch", C.c_int32), ("frames", C.c_int32),
                ("k", C.c_int32), ("mx", C.c_int32), ("my", C.c_int32), ("ncx", C.c_int32), ("ncy", C.c_int32), ("d", C.c_float),
                ("flags", C.c_uint32)]


class SpectraDesc(C.Structure):
    _fields_ = [("nrows", C.c_int32), ("blocksize", C.c_int32), ("device", C.c_int32), ("max_batch", C.c_int32), ("frames", C.c_int32),
                ("nfft", C.c_int32), ("overlap", C.c_int32), ("window", C.c_int32), ("band_lo", C.c_int32), ("band_hi", C.c_int32)]


class CafDesc(C.Structure):
    _fields_ = [("nrows", C.c_int32), ("blocksize", C.c_int32), ("device", C.c_int32), ("max_batch", C.c_int32), ("frames", C.c_int32),
                ("seg", C.c_int32), ("nlags", C.c_int32), ("ref_row", C.c_int32), ("window", C.c_int32), ("guard", C.c_int32)]


class CfarDesc(C.Structure):
    """crsdr_cfar_desc: guard (gd, gr) and training (td, tr) half-widths over Doppler and lag, the threshold factor, the fewest
    training cells a detection needs, and K detections kept per map."""
    _fields_ = [("gd", C.c_int32), ("gr", C.c_int32), ("td", C.c_int32), ("tr", C.c_int32), ("alpha", C.c_float), ("min_train", C.c_int32),
                ("max_det", C.c_int32)]


CFAR_CA, CFAR_GO, CFAR_SO, CFAR_OS = 0, 1, 2, 3
CFAR_AXIS_LAG, CFAR_AXIS_DOPPLER = 0, 1


class CfarEstDesc(C.Structure):
    """crsdr_cfar_est_desc: the noise estimate (CFAR_CA, _GO, _SO, _OS), the axis that GO and SO split the training set over, the rank
    of OS among the Nfull cells of a whole window."""
    _fields_ = [("estimator", C.c_int32), ("axis", C.c_int32), ("rank", C.c_int32)]


class CancelDesc(C.Structure):
    """crsdr_caf_cancel_desc: the reference's delays 0 .. taps - 1, each shifted by -dopp .. dopp Doppler bins."""
    _fields_ = [("taps", C.c_int32), ("dopp", C.c_int32)]


class CleanDesc(C.Structure):
    """crsdr_caf_clean_desc: at most max_targets picks a line, none under min_snr, each a cluster of lags l - wl .. l + wl and Dopplers
    f - wq / 2 .. f + wq / 2 in steps of half a bin."""
    _fields_ = [("max_targets", C.c_int32), ("min_snr", C.c_float), ("wl", C.c_int32), ("wq", C.c_int32)]


CLEAN_KEYS = ("chi", "map", "peak", "coef", "cinfo", "det", "count", "snap", "tgt", "ntgt", "tcoef", "tinfo", "rchi", "rmap", "rdet", "rcount", "rsnap")


class CleanOut(C.Structure):
    """crsdr_clean_out: where crsdr_ambiguity_clean writes (NULL: not asked for)."""
    _fields_ = [(k, C.c_void_p) for k in CLEAN_KEYS]


class BearingDesc(C.Structure):
    """crsdr_caf_bearing_desc: the mx x my array of the rows other than the reference, the scan grid, the spacing in wavelengths, the
    mode with its loading, the zoom levels and the flags."""
    _fields_ = [("mx", C.c_int32), ("my", C.c_int32), ("ncx", C.c_int32), ("ncy", C.c_int32), ("d", C.c_float), ("mode", C.c_int32),
                ("loading", C.c_float), ("levels", C.c_int32), ("flags", C.c_uint32)]


class BeamsDesc(C.Structure):
    """crsdr_caf_beams_desc: nbeams weight rows [nbeams][m][2] float32 on the host (copied by the call), and the flags (none yet)."""
    _fields_ = [("nbeams", C.c_int32), ("weights", C.POINTER(C.c_float)), ("flags", C.c_uint32)]


class BeamAdaptDesc(C.Structure):
    """crsdr_caf_beam_adapt_desc: the training rectangle of a line -- Doppler bins (d_lo + a) mod nd, a < d_n, lags r_lo + b, b < r_n --
    the diagonal loading relative to trace(Q) / m, and the flags (none yet)."""
    _fields_ = [("d_lo", C.c_int32), ("d_n", C.c_int32), ("r_lo", C.c_int32), ("r_n", C.c_int32), ("loading", C.c_float), ("flags", C.c_uint32)]


class TrackDesc(C.Structure):
    """crsdr_caf_track_desc: the slots, the source list, the measurement deviations, the gate on d2, the new track's rate variance, the
    process noise per line, the lag-Doppler coupling, m-of-n confirmation and the misses that end a tentative and a confirmed track."""
    _fields_ = [("max_tracks", C.c_int32), ("source", C.c_int32), ("sigma_r", C.c_double), ("sigma_f", C.c_double), ("gate", C.c_double),
                ("p0_g", C.c_double), ("q_r", C.c_double), ("q_f", C.c_double), ("q_g", C.c_double), ("coupling", C.c_double),
                ("m", C.c_int32), ("n", C.c_int32), ("tent_miss", C.c_int32), ("conf_miss", C.c_int32)]


class IntegrateDesc(C.Structure):
    """crsdr_caf_integrate_desc: which maps (INTEGRATE_ARRAY, INTEGRATE_BEAMS), the forgetting factor in (0, 1] and the coupling in lag
    cells per line per Doppler bin (the tracker's figure)."""
    _fields_ = [("what", C.c_int32), ("reserved", C.c_int32), ("forget", C.c_double), ("coupling", C.c_double)]


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise FileNotFoundError(f"{_SO} is missing: run __graft_entry__.build() (hipcc) first; there is no CPU fallback")
    # A Python process that also uses PyTorch must load torch's bundled HIP runtime BEFORE this library: both
    # carry the soname libamdhip64.so.7, the first one loaded serves both, and torch's device init fails on the
    # system runtime.  (C / C++ hosts are not affected: they link one runtime.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(_SO)
    f32p, i8p, u8p, u32p, i32p, vp = (C.POINTER(C.c_float), C.POINTER(C.c_int8), C.POINTER(C.c_uint8),
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_void_p)
    L.crsdr_abi_version.restype = C.c_int
    L.crsdr_last_error.restype = C.c_char_p
    L.crsdr_device_count.argtypes = [C.POINTER(C.c_int)]
    L.crsdr_host_alloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    L.crsdr_host_free.argtypes = [C.c_void_p]
    L.crsdr_device_info.argtypes = [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    L.crsdr_convtosigned.argtypes = [u8p, u8p, C.c_int]
    L.crsdr_convtofloat.argtypes = [f32p, i8p, C.c_int]
    L.crsdr_scalarmul.argtypes = [f32p, f32p, C.c_float, C.c_float, C.c_int]
    L.crsdr_convto8bit.argtypes = [i8p, f32p, C.c_int]
    L.crsdr_conj_dotproduct.argtypes = [f32p, f32p, f32p, C.c_int]
    L.crsdr_magsquared.argtypes = [f32p, f32p, C.c_int]
    L.crsdr_conjugatemul.argtypes = [f32p, f32p, f32p, C.c_int]
    L.crsdr_indexofmax.argtypes = [u32p, f32p, C.c_int]
    L.crsdr_fft.argtypes = [f32p, f32p, C.c_int, C.c_int, C.c_int]
    L.crsdr_covariance.argtypes = [f32p, i8p, C.c_int, C.c_int, C.c_int]
    L.crsdr_noisesubspace.argtypes = [f32p, f32p, f32p, C.c_int, C.c_int]
    L.crsdr_pmusic2d.argtypes = [f32p, f32p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.crsdr_plan_create.argtypes = [C.POINTER(vp), C.POINTER(PlanDesc)]
    L.crsdr_plan_destroy.argtypes = [vp]
    L.crsdr_plan_reset.argtypes = [vp]
    L.crsdr_plan_set_stream.argtypes = [vp, vp]
    L.crsdr_plan_submit.argtypes = [vp, vp, C.c_int, u32p, u8p, C.c_uint32, C.c_uint32]
    L.crsdr_plan_fetch.argtypes = [vp, i32p, f32p, f32p, f32p, i8p]
    L.crsdr_plan_sync.argtypes = [vp]
    L.crsdr_plan_packet_bytes.argtypes = [vp]
    L.crsdr_plan_packet_bytes.restype = C.c_size_t
    L.crsdr_plan_matrix_offset.argtypes = [vp]
    L.crsdr_plan_matrix_offset.restype = C.c_size_t
    L.crsdr_plan_device_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.crsdr_plan_bind_packet.argtypes = [vp, vp, C.c_size_t]
    L.crsdr_plan_bind_slab.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int]
    L.crsdr_assemble_slabs.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp]
    L.crsdr_plan_submit_batch.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, u32p, u8p, C.c_uint32, C.c_uint32]
    szp = C.POINTER(C.c_size_t)
    L.crsdr_plan_set_frac_apply.argtypes = [vp, C.c_int, C.c_float, f32p]
    L.crsdr_plan_fetch_batch_async.argtypes = [vp, vp, vp, vp, vp, vp, C.c_size_t]
    L.crsdr_plan_fetch_wait.argtypes = [vp]
    L.crsdr_plan_bind_slab_ex.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_size_t]
    L.crsdr_exchange_geometry.argtypes = [C.c_int, C.c_int, C.c_int, szp, szp, szp]
    L.crsdr_exchange_rooted_blocks.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.crsdr_assemble_slots.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, vp, vp]
    L.crsdr_exchange_unique_id.argtypes = [vp]
    L.crsdr_exchange_create.argtypes = [C.POINTER(vp), vp, C.c_int, C.c_int, C.c_int]
    L.crsdr_exchange_destroy.argtypes = [vp]
    L.crsdr_exchange_batch.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, vp]
    L.crsdr_exchange_schedule.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(XOp), C.c_int, C.POINTER(C.c_int)]
    L.crsdr_exchange_bind_plan.argtypes = [vp, vp, C.c_int]
    L.crsdr_exchange_submit_batch.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, u32p, u8p, C.c_uint32, C.c_uint32]
    L.crsdr_exchange_fetch_rooted.argtypes = [vp, C.POINTER(C.c_int8), C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                              C.POINTER(C.c_int)]
    L.crsdr_plan_fetch_block.argtypes = [vp, C.c_int, i32p, f32p, f32p, f32p, i8p]
    L.crsdr_plan_packet_stride.argtypes = [vp]
    L.crsdr_plan_packet_stride.restype = C.c_size_t
    L.crsdr_plan_last_elapsed_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.crsdr_plan_enable_profiling.argtypes = [vp, C.c_int, C.c_uint32]
    L.crsdr_plan_kernel_times.argtypes = [vp, C.c_int, f32p, C.c_int, C.POINTER(C.c_int)]
    if hasattr(L, "crsdr_doa_create"):               # (CRSDR_LIB may name an older build for an A/B of the per-op calls)
        L.crsdr_doa_create.argtypes = [C.POINTER(vp), C.POINTER(DoaDesc)]
        L.crsdr_doa_destroy.argtypes = [vp]
        L.crsdr_doa_submit.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, vp]
        L.crsdr_doa_submit_plan.argtypes = [vp, vp]
        L.crsdr_doa_fetch.argtypes = [vp, i32p, f32p, f32p, i32p, f32p, f32p]
        L.crsdr_doa_device_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.crsdr_doa_last_submit.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if hasattr(L, "crsdr_doa_set_peaks"):            # (likewise: an older build has the engine without the local-peak pass)
        L.crsdr_doa_set_peaks.argtypes = [vp, C.c_int, C.c_int]
        L.crsdr_doa_fetch_directions.argtypes = [vp, i32p, i32p, f32p]
        L.crsdr_doa_direction_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    if hasattr(L, "crsdr_doa_set_beams"):            # (likewise: an older build has no beams)
        L.crsdr_beamform.argtypes = [f32p, i8p, C.c_int, C.c_int, f32p, C.c_int, C.c_int]
        L.crsdr_doa_set_beams.argtypes = [vp, C.c_int, C.c_float, C.c_int, f32p]
        L.crsdr_doa_fetch_beams.argtypes = [vp, f32p, f32p, f32p]
        L.crsdr_doa_beam_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int)]
        L.crsdr_doa_fetch_subspace.argtypes = [vp, f32p]
    if hasattr(L, "crsdr_doa_set_smoothing"):        # (likewise: an older build has neither smoothing nor the source count)
        L.crsdr_doa_set_smoothing.argtypes = [vp, C.c_int, C.c_int, C.c_uint32]
        L.crsdr_doa_fetch_smoothed.argtypes = [vp, f32p]
        L.crsdr_doa_set_order.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
        L.crsdr_doa_fetch_order.argtypes = [vp, i32p, f32p]
        L.crsdr_doa_order_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    if hasattr(L, "crsdr_doa_set_subbands"):         # (likewise: an older build has no subbands)
        L.crsdr_doa_set_subbands.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.crsdr_doa_fetch_subbands.argtypes = [vp, f32p]
        L.crsdr_doa_subband_buffers.argtypes = [vp, C.POINTER(vp)]
        L.crsdr_subband_covariance.argtypes = [f32p, f32p, i8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.crsdr_smooth_covariance.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int]
        L.crsdr_source_order.argtypes = [vp, vp, vp, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]
    if hasattr(L, "crsdr_doa_set_subband_beams"):    # (likewise: an older build has no band beams)
        L.crsdr_doa_set_subband_beams.argtypes = [vp, C.c_int, C.c_float, C.c_int, f32p]
        L.crsdr_doa_fetch_subband_beams.argtypes = [vp, f32p, f32p, f32p]
        L.crsdr_doa_subband_beam_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int)]
        L.crsdr_subband_beamform.argtypes = [f32p, i8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_int]
    if hasattr(L, "crsdr_doa_set_spectrum"):         # (likewise: an older build has the MUSIC map alone)
        L.crsdr_doa_set_spectrum.argtypes = [vp, C.c_int, C.c_float]
        L.crsdr_spectrum2d.argtypes = [f32p, f32p, f32p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    if hasattr(L, "crsdr_doa_set_refine"):           # (likewise: an older build reports grid points alone)
        L.crsdr_doa_set_refine.argtypes = [vp, C.c_int]
        L.crsdr_doa_fetch_refined.argtypes = [vp, f32p, f32p, f32p]
        L.crsdr_doa_refined_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int)]
        L.crsdr_refine2d.argtypes = [f32p, f32p, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, i32p,
                                     C.c_int, C.c_int, C.c_int]
    if hasattr(L, "crsdr_doa_set_esprit"):           # (likewise: an older build has the scans alone)
        f64p = C.POINTER(C.c_double)
        L.crsdr_doa_set_esprit.argtypes = [vp, C.c_int]
        L.crsdr_doa_fetch_esprit.argtypes = [vp, i32p, i32p, f64p, f32p, f32p, f32p, i32p]
        L.crsdr_doa_esprit_buffers.argtypes = [vp] + [C.POINTER(vp)] * 7 + [C.POINTER(C.c_int)]
        L.crsdr_esprit2d.argtypes = [i32p, i32p, f64p, f32p, f32p, f32p, i32p, f32p, f32p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int]
    if hasattr(L, "crsdr_doa_set_augment"):          # (likewise: an older build has no augmentation)
        L.crsdr_doa_set_augment.argtypes = [vp, C.c_int, C.c_int, C.c_uint64]
        L.crsdr_doa_fetch_augmented.argtypes = [vp, f32p]
        L.crsdr_doa_augment_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.crsdr_augment_covariance.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int]
        L.crsdr_augment_lags.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, i32p, C.POINTER(C.c_int)]
    if hasattr(L, "crsdr_plan_set_refcancel"):       # (likewise: an older build has no reference-noise canceller)
        L.crsdr_plan_set_refcancel.argtypes = [vp, C.c_int]
        L.crsdr_plan_fetch_refcancel.argtypes = [vp, C.c_int, f32p, f32p, i32p]
        L.crsdr_plan_refcancel_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int)]
        L.crsdr_refcancel.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_uint32, C.c_int]
    if hasattr(L, "crsdr_spectra_create"):           # (likewise: an older build has no spectra)
        L.crsdr_spectra_create.argtypes = [C.POINTER(vp), C.POINTER(SpectraDesc)]
        L.crsdr_spectra_destroy.argtypes = [vp]
        L.crsdr_spectra_submit.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, vp]
        L.crsdr_spectra_submit_plan.argtypes = [vp, vp]
        L.crsdr_spectra_fetch.argtypes = [vp, f32p, f32p, f32p]
        L.crsdr_spectra_device_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.crsdr_spectra_last_submit.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.crsdr_welch.argtypes = [f32p, f32p, f32p, i8p] + [C.c_int] * 8
    if hasattr(L, "crsdr_caf_create"):               # (likewise: an older build has no range-Doppler maps)
        L.crsdr_caf_create.argtypes = [C.POINTER(vp), C.POINTER(CafDesc)]
        L.crsdr_caf_destroy.argtypes = [vp]
        L.crsdr_caf_submit.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, vp]
        L.crsdr_caf_submit_plan.argtypes = [vp, vp]
        L.crsdr_caf_fetch.argtypes = [vp, f32p, f32p, f32p]
        L.crsdr_caf_device_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.crsdr_caf_last_submit.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.crsdr_ambiguity.argtypes = [f32p, f32p, f32p, i8p] + [C.c_int] * 8
    if hasattr(L, "crsdr_cfar"):                     # (likewise: an older build has no detector)
        L.crsdr_caf_set_cfar.argtypes = [vp, C.POINTER(CfarDesc)]
        L.crsdr_caf_fetch_cfar.argtypes = [vp, f32p, i32p, f32p]
        L.crsdr_caf_cfar_device_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.crsdr_cfar.argtypes = [f32p, i32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(CfarDesc), C.c_int]
        L.crsdr_cfar_alpha.argtypes = [C.c_double, C.c_int, f32p]
    if hasattr(L, "crsdr_cfar_est"):                 # (likewise: an older build knows cell averaging alone)
        L.crsdr_caf_set_cfar_estimator.argtypes = [vp, C.POINTER(CfarEstDesc)]
        L.crsdr_cfar_est.argtypes = [f32p, i32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(CfarDesc), C.POINTER(CfarEstDesc), C.c_int]
        L.crsdr_cfar_alpha_est.argtypes = [C.c_double, C.c_int, C.POINTER(CfarEstDesc), f32p]
    if hasattr(L, "crsdr_ambiguity_cancel"):         # (likewise: an older build has no canceller)
        L.crsdr_caf_set_cancel.argtypes = [vp, C.POINTER(CancelDesc)]
        L.crsdr_caf_fetch_cancel.argtypes = [vp, f32p, f32p]
        L.crsdr_caf_cancel_device_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        L.crsdr_ambiguity_cancel.argtypes = [f32p, f32p, f32p, C.POINTER(C.c_int8)] + [C.c_int] * 10 + [f32p, f32p]
    if hasattr(L, "crsdr_bearing"):                  # (likewise: an older build has no bearings)
        L.crsdr_caf_set_bearing.argtypes = [vp, C.POINTER(BearingDesc)]
        L.crsdr_caf_fetch_bearing.argtypes = [vp, f32p, f32p]
        L.crsdr_caf_bearing_device_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        L.crsdr_bearing.argtypes = [f32p, f32p, f32p] + [C.c_int] * 5 + [f32p, i32p, C.POINTER(CfarDesc), C.POINTER(BearingDesc), C.c_int]
    if hasattr(L, "crsdr_beam_maps"):                # (likewise: an older build has no beams)
        L.crsdr_caf_set_beams.argtypes = [vp, C.POINTER(BeamsDesc)]
        L.crsdr_caf_fetch_beams.argtypes = [vp, f32p, f32p, i32p, f32p, i32p]
        L.crsdr_caf_beams_device_buffers.argtypes = [vp] + [C.POINTER(vp)] * 5
        L.crsdr_beam_maps.argtypes = [f32p, f32p] + [C.c_int] * 4 + [f32p, C.c_int, C.c_int]
        L.crsdr_beam_fuse.argtypes = [f32p, i32p, f32p, i32p] + [C.c_int] * 5
        L.crsdr_caf_beam_steer.argtypes = [f32p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int]
    if hasattr(L, "crsdr_beam_adapt"):               # (likewise: an older build has no adaptive beams)
        L.crsdr_caf_set_beam_adapt.argtypes = [vp, C.POINTER(BeamAdaptDesc)]
        L.crsdr_caf_fetch_beam_adapt.argtypes = [vp, f32p, f32p, i32p]
        L.crsdr_caf_beam_adapt_device_buffers.argtypes = [vp] + [C.POINTER(vp)] * 3
        L.crsdr_beam_adapt.argtypes = [f32p, f32p, i32p, f32p] + [C.c_int] * 4 + [f32p, C.c_int, C.POINTER(BeamAdaptDesc), C.c_int]
    if hasattr(L, "crsdr_track"):                    # (likewise: an older build has no tracker)
        L.crsdr_caf_set_track.argtypes = [vp, C.POINTER(TrackDesc)]
        L.crsdr_caf_track_reset.argtypes = [vp]
        L.crsdr_caf_fetch_track.argtypes = [vp, f32p, i32p]
        L.crsdr_caf_track_device_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        L.crsdr_track_state_bytes.argtypes = [C.POINTER(TrackDesc), C.POINTER(C.c_size_t)]
        L.crsdr_track.argtypes = [f32p, i32p, vp, f32p, i32p, f32p] + [C.c_int] * 4 + [C.POINTER(TrackDesc), C.c_int]
    if hasattr(L, "crsdr_ambiguity_clean"):          # (likewise: an older build has no second cancellation stage)
        L.crsdr_caf_set_clean.argtypes = [vp, C.POINTER(CleanDesc)]
        L.crsdr_caf_fetch_clean.argtypes = [vp, f32p, i32p, f32p, f32p, f32p, f32p, f32p, i32p, f32p]
        L.crsdr_caf_clean_device_buffers.argtypes = [vp] + [C.POINTER(vp)] * 9
        L.crsdr_ambiguity_clean.argtypes = [C.POINTER(CleanOut), C.POINTER(C.c_int8)] + [C.c_int] * 8 + [C.POINTER(CancelDesc), C.POINTER(CfarDesc), C.POINTER(CfarEstDesc),
                                                                                                         C.POINTER(CleanDesc)]
    if hasattr(L, "crsdr_map_integrate"):            # (likewise: an older build has no integration across lines)
        L.crsdr_caf_set_integrate.argtypes = [vp, C.POINTER(IntegrateDesc)]
        L.crsdr_caf_integrate_reset.argtypes = [vp]
        L.crsdr_caf_fetch_integrate.argtypes = [vp, f32p, f32p]
        L.crsdr_caf_integrate_device_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.crsdr_map_integrate_state_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        L.crsdr_map_integrate.argtypes = [f32p, vp, f32p] + [C.c_int] * 4 + [C.POINTER(IntegrateDesc), C.c_int]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise CrsdrError(rc, lib().crsdr_last_error().decode(errors="replace"))


def _p(a, ty):
    return a.ctypes.data_as(C.POINTER(ty)) if a is not None else None


def _c64(a):
    a = np.ascontiguousarray(a, dtype=np.complex64)
    return a, a.view(np.float32)


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().crsdr_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def device_info(device: int = 0) -> dict:
    name = C.create_string_buffer(256)
    cus, clk, mclk, mem = C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0)
    _check(lib().crsdr_device_info(int(device), name, 256, C.byref(cus), C.byref(clk), C.byref(mclk), C.byref(mem)))
    return {"name": name.value.decode(errors="replace"), "compute_units": cus.value, "clock_mhz": clk.value / 1e3,
            "memory_clock_mhz": mclk.value / 1e3, "memory_gib": round(mem.value / 2**30, 1)}


class PinnedArray:
    """numpy view of page-locked host memory from crsdr_host_alloc (freed on close / garbage collection)."""

    def __init__(self, shape, dtype=np.int8):
        self.shape, self.dtype = tuple(np.atleast_1d(shape)), np.dtype(dtype)
        nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self._ptr = C.c_void_p()
        _check(lib().crsdr_host_alloc(C.byref(self._ptr), nbytes))
        self.array = np.frombuffer((C.c_uint8 * nbytes).from_address(self._ptr.value), dtype=self.dtype).reshape(self.shape)

    def close(self):
        if self._ptr:
            self.array = None
            lib().crsdr_host_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- per-op wrappers (class cdsp), numpy host arrays in / out ----------------------------------

def convtosigned(u8):
    u8 = np.ascontiguousarray(u8, dtype=np.uint8)
    out = np.empty_like(u8)
    _check(lib().crsdr_convtosigned(_p(u8, C.c_uint8), _p(out, C.c_uint8), u8.size))
    return out.view(np.int8)


def convtofloat(i8):
    i8 = np.ascontiguousarray(i8, dtype=np.int8)
    out = np.empty(i8.size, dtype=np.float32)
    _check(lib().crsdr_convtofloat(_p(out, C.c_float), _p(i8, C.c_int8), i8.size))
    return out.view(np.complex64)


def scalarmul(x, s):
    x, xf = _c64(x)
    out = np.empty_like(x)
    s = np.complex64(s)
    _check(lib().crsdr_scalarmul(_p(out.view(np.float32), C.c_float), _p(xf, C.c_float), float(s.real), float(s.imag), x.size))
    return out


def convto8bit(x):
    x, xf = _c64(x)
    out = np.empty(2 * x.size, dtype=np.int8)
    _check(lib().crsdr_convto8bit(_p(out, C.c_int8), _p(xf, C.c_float), x.size))
    return out


def conj_dotproduct(a, b):
    a, af = _c64(a)
    b, bf = _c64(b)
    res = np.zeros(2, dtype=np.float32)
    _check(lib().crsdr_conj_dotproduct(_p(res, C.c_float), _p(af, C.c_float), _p(bf, C.c_float), a.size))
    return np.complex64(res[0] + 1j * res[1])


def magsquared(x):
    x, xf = _c64(x)
    out = np.empty(x.size, dtype=np.float32)
    _check(lib().crsdr_magsquared(_p(out, C.c_float), _p(xf, C.c_float), x.size))
    return out


def conjugatemul(a, b):
    a, af = _c64(a)
    b, bf = _c64(b)
    out = np.empty_like(a)
    _check(lib().crsdr_conjugatemul(_p(out.view(np.float32), C.c_float), _p(af, C.c_float), _p(bf, C.c_float), a.size))
    return out


def indexofmax(m):
    m = np.ascontiguousarray(m, dtype=np.float32)
    idx = C.c_uint32(0)
    _check(lib().crsdr_indexofmax(C.byref(idx), _p(m, C.c_float), m.size))
    return int(idx.value)


def fft(x, sign=-1):
    x, xf = _c64(x)
    n = x.shape[-1]
    out = np.empty_like(x)
    _check(lib().crsdr_fft(_p(out.view(np.float32), C.c_float), _p(xf, C.c_float), n, sign, x.size // n))
    return out


def covariance(matrix):
    """Rxx of the signal rows of an aligned int8 matrix [nrows][B] (beamformer's first step)."""
    m = np.ascontiguousarray(matrix, dtype=np.int8)
    nrows, B = m.shape
    out = np.empty((nrows - 1, nrows - 1), dtype=np.complex64)
    _check(lib().crsdr_covariance(_p(out.view(np.float32), C.c_float), _p(m, C.c_int8), nrows, B, MEM_HOST))
    return out


def refcancel(rows, lag, phasor, taps, flags=0):
    """crsdr_refcancel: the reference-noise canceller on one block rows [nrows][B] (int8, or uint8 with OFFSET_BINARY) with the lags
    [nrows] and phasors [nrows] given.  Returns dict(out [nrows][B] int8, coef [nrows][taps] complex64, residual [nrows], status [nrows])."""
    r = np.ascontiguousarray(rows)
    if r.dtype not in (np.int8, np.uint8) or r.ndim != 2:
        raise TypeError("rows must be int8 (or offset-binary uint8) [nrows][B]")
    nrows, B = r.shape
    lg = np.ascontiguousarray(lag, dtype=np.int32)
    ph = np.ascontiguousarray(phasor, dtype=np.complex64)
    if lg.shape != (nrows,) or ph.shape != (nrows,):
        raise ValueError("lag and phasor must be [nrows]")
    out = np.zeros((nrows, B), dtype=np.int8)
    coef = np.zeros((nrows, max(int(taps), 1)), dtype=np.complex64)
    res, st = np.zeros(nrows, dtype=np.float32), np.zeros(nrows, dtype=np.int32)
    _check(lib().crsdr_refcancel(out.ctypes.data, coef.ctypes.data, res.ctypes.data, st.ctypes.data, r.ctypes.data, nrows, B, lg.ctypes.data,
                                 ph.ctypes.data, int(taps), int(flags), MEM_HOST))
    return dict(out=out, coef=coef, residual=res, status=st)


def refcancel_device(out_ptr, coef_ptr, residual_ptr, status_ptr, rows_ptr, nrows, B, lag_ptr, phasor_ptr, taps, flags=0):
    """Same on device memory (every pointer on the current device); returns after the kernels finished."""
    _check(lib().crsdr_refcancel(int(out_ptr), int(coef_ptr), int(residual_ptr), int(status_ptr), int(rows_ptr), int(nrows), int(B), int(lag_ptr),
                                 int(phasor_ptr), int(taps), int(flags), MEM_DEVICE))


def covariance_device(rxx_ptr: int, matrix_ptr: int, nrows: int, B: int):
    """Same on device memory (both pointers on the current device); returns after the kernels finished."""
    _check(lib().crsdr_covariance(C.cast(C.c_void_p(int(rxx_ptr)), C.POINTER(C.c_float)),
                                  C.cast(C.c_void_p(int(matrix_ptr)), C.POINTER(C.c_int8)), nrows, B, MEM_DEVICE))


def noisesubspace(rxx):
    """noisesubspace(Rxx, K) of beamformclient/heatmap2d2.cpp:69-79 without the column cut: returns (vec, sv) with
    vec[:, r] the singular vector of sv[r], sv descending; the noise subspace for K sources is vec[:, K:]."""
    r = np.ascontiguousarray(rxx, dtype=np.complex64)
    if r.ndim != 2 or r.shape[0] != r.shape[1]:
        raise ValueError("rxx must be square")
    M = r.shape[0]
    vec = np.empty((M, M), dtype=np.complex64)
    sv = np.empty(M, dtype=np.float32)
    _check(lib().crsdr_noisesubspace(_p(vec.view(np.float32), C.c_float), _p(sv, C.c_float), _p(r.view(np.float32), C.c_float), M, MEM_HOST))
    return vec, sv


def pmusic2d(vec, k, d, mx, my, ncx=100, ncy=100):
    """pmusic2dvec(Un, d, Mx, My, Cx, Cy) of beamformclient/heatmap2d2.cpp:137-147 with Un = vec[:, k:]."""
    v = np.ascontiguousarray(vec, dtype=np.complex64)
    M = v.shape[0]
    pm = np.empty((max(ncx, 0), max(ncy, 0)), dtype=np.float32)
    _check(lib().crsdr_pmusic2d(_p(pm, C.c_float), _p(v.view(np.float32), C.c_float), M, int(k), C.c_float(d), int(mx), int(my),
                                int(ncx), int(ncy), MEM_HOST))
    return pm


def spectrum2d(vec, sv, kind, d, mx, my, ncx=100, ncy=100, loading=1e-2):
    """crsdr_spectrum2d: the Bartlett (SPECTRUM_BARTLETT) or Capon (SPECTRUM_CAPON, with its diagonal loading) power map
    pm [ncx][ncy] of the subspace (vec, sv) as noisesubspace returns it, over the grid and with the steering vector of pmusic2d."""
    v = np.ascontiguousarray(vec, dtype=np.complex64)
    s = np.ascontiguousarray(sv, dtype=np.float32)
    M = v.shape[0]
    if v.shape != (M, M) or s.shape != (M,):
        raise ValueError("vec must be [m][m] and sv [m]")
    pm = np.empty((max(ncx, 0), max(ncy, 0)), dtype=np.float32)
    _check(lib().crsdr_spectrum2d(_p(pm, C.c_float), _p(v.view(np.float32), C.c_float), _p(s, C.c_float), M, int(kind), C.c_float(loading),
                                  C.c_float(d), int(mx), int(my), int(ncx), int(ncy), MEM_HOST))
    return pm


def spectrum2d_device(pm_ptr: int, vec_ptr: int, sv_ptr: int, m, kind, d, mx, my, ncx=100, ncy=100, loading=1e-2):
    """Same on device memory (all three pointers on the current device); returns after the kernel finished."""
    f32p = C.POINTER(C.c_float)
    _check(lib().crsdr_spectrum2d(C.cast(C.c_void_p(int(pm_ptr)), f32p), C.cast(C.c_void_p(int(vec_ptr)), f32p), C.cast(C.c_void_p(int(sv_ptr)), f32p),
                                  int(m), int(kind), C.c_float(loading), C.c_float(d), int(mx), int(my), int(ncx), int(ncy), MEM_DEVICE))


def refine2d(vec, sv, kind, peaks, d, mx, my, ncx=100, ncy=100, k=1, loading=1e-2, levels=5):
    """crsdr_refine2d: the directions peaks [n][2] (cx, cy) of the map `kind` (SPECTRUM_*; k: MUSIC's sources, loading: Capon's) of the
    subspace (vec, sv), refined off the grid by `levels` levels of the zoom search.  offsets [n][2] in grid cells, angles [n][2]
    (alpha, beta) in radians, values [n]."""
    v = np.ascontiguousarray(vec, dtype=np.complex64)
    s = np.ascontiguousarray(sv, dtype=np.float32)
    pk = np.ascontiguousarray(peaks, dtype=np.int32).reshape(-1, 2)
    M, n = v.shape[0], pk.shape[0]
    if v.shape != (M, M) or s.shape != (M,):
        raise ValueError("vec must be [m][m] and sv [m]")
    off, ang, val = np.zeros((n, 2), dtype=np.float32), np.zeros((n, 2), dtype=np.float32), np.zeros(n, dtype=np.float32)
    _check(lib().crsdr_refine2d(_p(off, C.c_float), _p(ang, C.c_float), _p(val, C.c_float), _p(v.view(np.float32), C.c_float), _p(s, C.c_float), M, int(kind),
                                int(k), C.c_float(loading), C.c_float(d), int(mx), int(my), int(ncx), int(ncy), _p(pk, C.c_int32), n, int(levels), MEM_HOST))
    return {"offsets": off, "angles": ang, "values": val}


def esprit2d(vec, sv, k, d, mx, my):
    """crsdr_esprit2d: the k directions of the subspace (vec, sv) of an mx x my array by 2-D ESPRIT, no grid.  found, status; phases [k][2]
    float64 (mu, nu); angles [k][2] (alpha, beta) in radians; modulus [k][2]; power [k]; flags [k]."""
    v = np.ascontiguousarray(vec, dtype=np.complex64)
    s = np.ascontiguousarray(sv, dtype=np.float32)
    M, n = v.shape[0], max(int(k), 0)
    if v.shape != (M, M) or s.shape != (M,):
        raise ValueError("vec must be [m][m] and sv [m]")
    found, status = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    ph, ang, mod = np.zeros((n, 2), dtype=np.float64), np.zeros((n, 2), dtype=np.float32), np.zeros((n, 2), dtype=np.float32)
    pw, fl = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32)
    _check(lib().crsdr_esprit2d(_p(found, C.c_int32), _p(status, C.c_int32), _p(ph, C.c_double), _p(ang, C.c_float), _p(mod, C.c_float), _p(pw, C.c_float),
                                _p(fl, C.c_int32), _p(v.view(np.float32), C.c_float), _p(s, C.c_float), M, int(k), C.c_float(d), int(mx), int(my), MEM_HOST))
    return {"found": int(found[0]), "status": int(status[0]), "phases": ph, "angles": ang, "modulus": mod, "power": pw, "flags": fl}


def beamform(matrix, weights):
    """crsdr_beamform: out [nbeams][B / 2] complex64 = weights [nbeams][nrows - 1] applied to the signal rows of matrix [nrows][B] int8
    (sum_c u[c - 1] (I_c + j Q_c) / 127, no conjugate): the batched engine's beam arithmetic on one matrix."""
    m = np.ascontiguousarray(matrix, dtype=np.int8)
    w = np.ascontiguousarray(weights, dtype=np.complex64)
    nrows, B = m.shape
    if w.ndim != 2 or w.shape[1] != nrows - 1:
        raise ValueError("weights must be [nbeams][nrows - 1]")
    out = np.empty((w.shape[0], B // 2), dtype=np.complex64)
    _check(lib().crsdr_beamform(_p(out.view(np.float32), C.c_float), _p(m, C.c_int8), nrows, B, _p(w.view(np.float32), C.c_float), w.shape[0], MEM_HOST))
    return out


def smooth_covariance(rxx, mx, my, sx, sy, flags=0):
    """crsdr_smooth_covariance: rs [sx sy][sx sy] complex64, the covariance rxx [mx my][mx my] averaged over its sx x sy sub-arrays
    (and with its backward image: SMOOTH_FB): the batched engine's smoothing on one matrix."""
    r = np.ascontiguousarray(rxx, dtype=np.complex64)
    if r.shape != (mx * my, mx * my):
        raise ValueError("rxx must be [mx * my][mx * my]")
    rs = np.empty((max(sx * sy, 0), max(sx * sy, 0)), dtype=np.complex64)
    _check(lib().crsdr_smooth_covariance(rs.ctypes.data, r.ctypes.data, int(mx), int(my), int(sx), int(sy), int(flags), MEM_HOST))
    return rs


def smooth_covariance_device(rs_ptr: int, rxx_ptr: int, mx, my, sx, sy, flags=0):
    """Same on device memory (both pointers on the current device); returns after the kernel finished."""
    _check(lib().crsdr_smooth_covariance(int(rs_ptr), int(rxx_ptr), int(mx), int(my), int(sx), int(sy), int(flags), MEM_DEVICE))


def mask_bits(mask) -> int:
    """The uint64 of an element mask: an int as it is, a string of '0' / '1' in element order (element i is character i), or an
    iterable of the indices that are present.  0 / None / "": all elements."""
    if mask is None:
        return 0
    if isinstance(mask, str):
        if set(mask) - {"0", "1"}:
            raise ValueError("a mask string holds only '0' and '1'")
        return sum(1 << i for i, ch in enumerate(mask) if ch == "1")
    if isinstance(mask, (int, np.integer)):
        return int(mask)
    return sum(1 << int(i) for i in mask)


def augment_covariance(rxx, mx, my, vx, vy, mask=0):
    """crsdr_augment_covariance: ra [vx vy][vx vy] complex64, the covariance of the filled vx x vy virtual array from the per-lag averages
    of rxx [mx my][mx my] over the elements of `mask` (mask_bits; 0: all): the batched engine's augmentation on one matrix."""
    r = np.ascontiguousarray(rxx, dtype=np.complex64)
    if r.shape != (mx * my, mx * my):
        raise ValueError("rxx must be [mx * my][mx * my]")
    mv = max(int(vx) * int(vy), 0)
    ra = np.empty((mv, mv), dtype=np.complex64)
    _check(lib().crsdr_augment_covariance(ra.ctypes.data, r.ctypes.data, int(mx), int(my), int(vx), int(vy), mask_bits(mask), MEM_HOST))
    return ra


def augment_covariance_device(ra_ptr: int, rxx_ptr: int, mx, my, vx, vy, mask=0):
    """Same on device memory (both pointers on the current device); returns after the kernel finished."""
    _check(lib().crsdr_augment_covariance(int(ra_ptr), int(rxx_ptr), int(mx), int(my), int(vx), int(vy), mask_bits(mask), MEM_DEVICE))


def augment_lags(mx, my, vx, vy, mask=0):
    """crsdr_augment_lags (host arithmetic, no device): (counts [vy][2 vx - 1] int32 with c(u) at [uy][ux + vx - 1], the number of
    uncovered half-plane lags)."""
    counts = np.zeros((max(int(vy), 1), max(2 * int(vx) - 1, 1)), dtype=np.int32)
    missing = C.c_int(0)
    _check(lib().crsdr_augment_lags(int(mx), int(my), int(vx), int(vy), mask_bits(mask), _p(counts, C.c_int32), C.byref(missing)))
    return counts, missing.value


def source_order(sv, nsnap, criterion=ORDER_MDL, kmin=1, kmax=None):
    """crsdr_source_order: (k, criterion values [kmax - kmin + 1]) from the singular values sv [m] of nsnap snapshots (ORDER_MDL /
    ORDER_AIC over k in kmin .. kmax, kmax = m - 1 by default): the batched engine's source count on one estimate."""
    s = np.ascontiguousarray(sv, dtype=np.float32)
    kmax = s.size - 1 if kmax is None else int(kmax)
    k, crit = np.zeros(1, dtype=np.int32), np.zeros(max(kmax - int(kmin) + 1, 1), dtype=np.float32)
    _check(lib().crsdr_source_order(k.ctypes.data, crit.ctypes.data, s.ctypes.data, s.size, int(nsnap), int(criterion), int(kmin), kmax, MEM_HOST))
    return int(k[0]), crit


def source_order_device(k_ptr: int, crit_ptr: int, sv_ptr: int, m, nsnap, criterion, kmin, kmax):
    """Same on device memory (crit_ptr may be 0); returns after the kernel finished."""
    _check(lib().crsdr_source_order(int(k_ptr), int(crit_ptr) or None, int(sv_ptr), int(m), int(nsnap), int(criterion), int(kmin), int(kmax), MEM_DEVICE))


def subband_covariance(matrix, nfft, first=0, nbands=1, width=1, window=WINDOW_RECT):
    """crsdr_subband_covariance: (rbands [nbands][m][m] complex64, power [nbands]) of one packet's int8 matrix [nrows][B]: band i
    is the sum of the per-bin covariances R_f over the bins (first + i width + u) mod nfft: the batched engine's subband covariance
    on one estimate of one packet."""
    m = np.ascontiguousarray(matrix, dtype=np.int8)
    nrows, B = m.shape
    rb = np.empty((max(int(nbands), 0), nrows - 1, nrows - 1), dtype=np.complex64)
    pw = np.empty(max(int(nbands), 0), dtype=np.float32)
    _check(lib().crsdr_subband_covariance(_p(rb.view(np.float32), C.c_float), _p(pw, C.c_float), _p(m, C.c_int8), nrows, B, int(nfft), int(first),
                                          int(nbands), int(width), int(window), MEM_HOST))
    return rb, pw


def subband_covariance_device(rbands_ptr: int, power_ptr: int, matrix_ptr: int, nrows, B, nfft, first, nbands, width, window):
    """Same on device memory (power_ptr may be 0); returns after the kernels finished."""
    cast = lambda p, t: C.cast(C.c_void_p(int(p) or None), C.POINTER(t))
    _check(lib().crsdr_subband_covariance(cast(rbands_ptr, C.c_float), cast(power_ptr, C.c_float), cast(matrix_ptr, C.c_int8), int(nrows), int(B),
                                          int(nfft), int(first), int(nbands), int(width), int(window), MEM_DEVICE))


def welch(matrix, nfft, overlap=0, window=WINDOW_RECT, band=None):
    """crsdr_welch: (psd [nrows][nfft] float32, cross [nrows][nfft] complex64, align [nrows][4] float32 = delay, phase, gain, coherence)
    of one packet's int8 matrix [nrows][B], row 0 included; band = (lo, hi) signed bins of the alignment figures (default +-nfft/4).
    The batched engine (Spectra) on one line of one packet, bit for bit."""
    m = np.ascontiguousarray(matrix, dtype=np.int8)
    nrows, B = m.shape
    lo, hi = band if band is not None else (-(int(nfft) // 4), int(nfft) // 4)
    n = max(int(nfft), 0)
    psd, cross, al = np.empty((nrows, n), dtype=np.float32), np.empty((nrows, n), dtype=np.complex64), np.empty((nrows, 4), dtype=np.float32)
    _check(lib().crsdr_welch(_p(psd, C.c_float), _p(cross.view(np.float32), C.c_float), _p(al, C.c_float), _p(m, C.c_int8), nrows, B, int(nfft), int(overlap),
                             int(window), int(lo), int(hi), MEM_HOST))
    return psd, cross, al


def welch_device(psd_ptr: int, cross_ptr: int, align_ptr: int, matrix_ptr: int, nrows, B, nfft, overlap, window, band_lo, band_hi):
    """Same on device memory (any output pointer, not all, may be 0); returns after the kernels finished."""
    cast = lambda p, t: C.cast(C.c_void_p(int(p) or None), C.POINTER(t))
    _check(lib().crsdr_welch(cast(psd_ptr, C.c_float), cast(cross_ptr, C.c_float), cast(align_ptr, C.c_float), cast(matrix_ptr, C.c_int8), int(nrows), int(B),
                             int(nfft), int(overlap), int(window), int(band_lo), int(band_hi), MEM_DEVICE))


def ambiguity(matrix, seg, nlags, ref_row=0, window=WINDOW_RECT, guard=0):
    """crsdr_ambiguity: (chi [nrows][nd][nlags] complex64, map [nd][nlags] float32, peak [nrows + 1][6] float32 = lag, doppler, power,
    ratio, dlag, ddop) of one packet's int8 matrix [nrows][B] against its row ref_row, nd = B / (2 seg) Doppler bins in FFT order.
    The batched engine (Caf) on one line of one packet, bit for bit."""
    m = np.ascontiguousarray(matrix, dtype=np.int8)
    nrows, B = m.shape
    nd, R = max(B // (2 * max(int(seg), 1)), 0), max(int(nlags), 0)
    chi, mp, pk = np.empty((nrows, nd, R), dtype=np.complex64), np.empty((nd, R), dtype=np.float32), np.empty((nrows + 1, 6), dtype=np.float32)
    _check(lib().crsdr_ambiguity(_p(chi.view(np.float32), C.c_float), _p(mp, C.c_float), _p(pk, C.c_float), _p(m, C.c_int8), nrows, B, int(seg), int(nlags),
                                 int(ref_row), int(window), int(guard), MEM_HOST))
    return chi, mp, pk


def cfar_desc(alpha, gd=1, gr=1, td=3, tr=4, min_train=1, max_det=16):
    return CfarDesc(int(gd), int(gr), int(td), int(tr), float(alpha), int(min_train), int(max_det))


def cfar_alpha(pfa, ntrain):
    """crsdr_cfar_alpha: ntrain (pfa^(-1 / ntrain) - 1) as a float32, the cell-averaging factor of one row's map."""
    a = C.c_float(0.0)
    _check(lib().crsdr_cfar_alpha(float(pfa), int(ntrain), C.byref(a)))
    return np.float32(a.value)


def cfar(src, guard, desc):
    """crsdr_cfar on ONE map: src [nd][R] float32 (a map) or complex64 (a chi) -> (det [K][8] float32 = lag, doppler, power, snr, noise,
    dlag, ddop, ntrain; count).  The engine's detector (Caf.set_cfar) on one map, bit for bit."""
    comps = 2 if np.iscomplexobj(src) else 1
    a = np.ascontiguousarray(src, dtype=np.complex64 if comps == 2 else np.float32)
    nd, R = a.shape
    det, count = np.zeros((desc.max_det, 8), dtype=np.float32), np.zeros(1, dtype=np.int32)
    _check(lib().crsdr_cfar(_p(det, C.c_float), _p(count, C.c_int32), _p(a.view(np.float32), C.c_float), comps, nd, R, int(guard), C.byref(desc), MEM_HOST))
    return det, int(count[0])


def cfar_device(det_ptr: int, count_ptr: int, src_ptr: int, comps, nd, R, guard, desc):
    """crsdr_cfar with CRSDR_MEM_DEVICE: every pointer on the device."""
    cast = lambda p, t: C.cast(C.c_void_p(int(p) or None), C.POINTER(t))
    _check(lib().crsdr_cfar(cast(det_ptr, C.c_float), cast(count_ptr, C.c_int32), cast(src_ptr, C.c_float), int(comps), int(nd), int(R), int(guard), C.byref(desc),
                            MEM_DEVICE))


def cfar_est_desc(estimator=CFAR_CA, axis=CFAR_AXIS_LAG, rank=0):
    return CfarEstDesc(int(estimator), int(axis), int(rank))


def cfar_alpha_est(pfa, ntrain, est):
    """crsdr_cfar_alpha_est: the alpha of a false-alarm probability pfa under exponential noise, from the estimator's exact equation.
    ntrain: the cells of one half (GO, SO) or of the whole training set (OS, CA)."""
    a = C.c_float(0.0)
    _check(lib().crsdr_cfar_alpha_est(float(pfa), int(ntrain), None if est is None else C.byref(est), C.byref(a)))
    return np.float32(a.value)


def cfar_est(src, guard, desc, est):
    """crsdr_cfar_est on ONE map: cfar() under the estimator est (None: cell averaging).  The engine's detector under
    Caf.set_cfar_estimator on one map, bit for bit."""
    comps = 2 if np.iscomplexobj(src) else 1
    a = np.ascontiguousarray(src, dtype=np.complex64 if comps == 2 else np.float32)
    nd, R = a.shape
    det, count = np.zeros((desc.max_det, 8), dtype=np.float32), np.zeros(1, dtype=np.int32)
    _check(lib().crsdr_cfar_est(_p(det, C.c_float), _p(count, C.c_int32), _p(a.view(np.float32), C.c_float), comps, nd, R, int(guard), C.byref(desc),
                                None if est is None else C.byref(est), MEM_HOST))
    return det, int(count[0])


def cfar_est_device(det_ptr: int, count_ptr: int, src_ptr: int, comps, nd, R, guard, desc, est):
    """crsdr_cfar_est with CRSDR_MEM_DEVICE: every pointer on the device."""
    cast = lambda p, t: C.cast(C.c_void_p(int(p) or None), C.POINTER(t))
    _check(lib().crsdr_cfar_est(cast(det_ptr, C.c_float), cast(count_ptr, C.c_int32), cast(src_ptr, C.c_float), int(comps), int(nd), int(R), int(guard), C.byref(desc),
                                None if est is None else C.byref(est), MEM_DEVICE))


def bearing_desc(mx, my, d, ncx=100, ncy=100, mode=BEARING_CONVENTIONAL, loading=1e-2, levels=0, flags=0):
    return BearingDesc(int(mx), int(my), int(ncx), int(ncy), float(d), int(mode), float(loading), int(levels), int(flags))


def bearing(chi, det, count, ref_row, guard, cfar, desc):
    """crsdr_bearing on ONE line: chi [nrows][nd][R] complex64, the array map's det [K][8] float32 and count as cfar() or Caf.fetch_cfar
    gave them -> (dir [K][8] float32 = cx, cy, T, dx, dy, alpha, beta, status; spec [K][ncx][ncy] float32 or None without
    BEARING_KEEP_SPECTRUM).  The engine's bearings (Caf.set_bearing) on one line, bit for bit."""
    a = np.ascontiguousarray(chi, dtype=np.complex64)
    nrows, nd, R = a.shape
    K = int(cfar.max_det)
    t = np.ascontiguousarray(det, dtype=np.float32).reshape(K, 8)
    n = np.array([count], dtype=np.int32).reshape(1)
    out = np.zeros((K, 8), dtype=np.float32)
    spec = np.zeros((K, desc.ncx, desc.ncy), dtype=np.float32) if desc.flags & BEARING_KEEP_SPECTRUM else None
    _check(lib().crsdr_bearing(_p(out, C.c_float), _p(spec, C.c_float), _p(a.view(np.float32), C.c_float), nrows, nd, R, int(ref_row), int(guard), _p(t, C.c_float),
                               _p(n, C.c_int32), C.byref(cfar), C.byref(desc), MEM_HOST))
    return out, spec


def bearing_device(dir_ptr: int, spec_ptr: int, chi_ptr: int, nrows, nd, R, ref_row, guard, det_ptr: int, count_ptr: int, cfar, desc):
    """crsdr_bearing with CRSDR_MEM_DEVICE: every pointer on the device (dir or spec, not both, may be 0)."""
    cast = lambda p, t: C.cast(C.c_void_p(int(p) or None), C.POINTER(t))
    _check(lib().crsdr_bearing(cast(dir_ptr, C.c_float), cast(spec_ptr, C.c_float), cast(chi_ptr, C.c_float), int(nrows), int(nd), int(R), int(ref_row), int(guard),
                               cast(det_ptr, C.c_float), cast(count_ptr, C.c_int32), C.byref(cfar), C.byref(desc), MEM_DEVICE))


def beams_desc(weights, flags=0):
    """crsdr_caf_beams_desc of weights [nbeams][m] complex (or [nbeams][m][2] float).  The descriptor keeps the float32 array alive."""
    w = np.asarray(weights)
    w = np.ascontiguousarray(w, dtype=np.complex64).view(np.float32) if np.iscomplexobj(w) else np.ascontiguousarray(w, dtype=np.float32)
    d = BeamsDesc(int(w.shape[0]), _p(w, C.c_float), int(flags))
    d._keep = w
    return d


def beam_steer(mx, my, d, xy, ncx=100, ncy=100):
    """crsdr_caf_beam_steer: weights [nbeams][mx my] complex64 = a(x, y) / sqrt(m) toward the cell coordinates xy [nbeams][2]."""
    pts = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    w = np.zeros((len(pts), max(int(mx) * int(my), 0)), dtype=np.complex64)
    _check(lib().crsdr_caf_beam_steer(_p(w.view(np.float32), C.c_float), int(mx), int(my), float(d), int(ncx), int(ncy), pts.ctypes.data_as(C.POINTER(C.c_double)), len(pts)))
    return w


def beam_maps(chi, weights, ref_row=0):
    """crsdr_beam_maps on ONE line: chi [nrows][nd][R] complex64, weights [nbeams][nrows - 1] complex64 -> bmap [nbeams][nd][R] float32.
    The engine's beam maps (Caf.set_beams) on one line, bit for bit."""
    a = np.ascontiguousarray(chi, dtype=np.complex64)
    w = np.ascontiguousarray(weights, dtype=np.complex64)
    nrows, nd, R = a.shape
    out = np.zeros((w.shape[0], nd, R), dtype=np.float32)
    _check(lib().crsdr_beam_maps(_p(out, C.c_float), _p(a.view(np.float32), C.c_float), nrows, nd, R, int(ref_row), _p(w.view(np.float32), C.c_float), int(w.shape[0]),
                                 MEM_HOST))
    return out


def beam_maps_device(bmap_ptr: int, chi_ptr: int, nrows, nd, R, ref_row, weights):
    """crsdr_beam_maps with CRSDR_MEM_DEVICE: bmap and chi on the device, the weights [nbeams][nrows - 1] complex64 on the host."""
    cast = lambda p, t: C.cast(C.c_void_p(int(p) or None), C.POINTER(t))
    w = np.ascontiguousarray(weights, dtype=np.complex64)
    _check(lib().crsdr_beam_maps(cast(bmap_ptr, C.c_float), cast(chi_ptr, C.c_float), int(nrows), int(nd), int(R), int(ref_row), _p(w.view(np.float32), C.c_float),
                                 int(w.shape[0]), MEM_DEVICE))


def beam_adapt_desc(loading, d_lo, d_n, r_lo, r_n, flags=0):
    return BeamAdaptDesc(int(d_lo), int(d_n), int(r_lo), int(r_n), float(loading), int(flags))


def beam_adapt(chi, weights, desc: "BeamAdaptDesc", ref_row=0):
    """crsdr_beam_adapt on ONE line: chi [nrows][nd][R] complex64, weights [nbeams][nrows - 1] complex64 -> (aw [nbeams][nrows - 1]
    complex64, ainfo [nbeams][2] float32, astat int).  The engine's adaptive weights (Caf.set_beam_adapt) on one line, bit for bit;
    beam_maps(chi, aw) is then the line's bmap."""
    a = np.ascontiguousarray(chi, dtype=np.complex64)
    w = np.ascontiguousarray(weights, dtype=np.complex64)
    nrows, nd, R = a.shape
    aw, info, stat = np.zeros(w.shape, dtype=np.complex64), np.zeros((w.shape[0], 2), dtype=np.float32), np.zeros(1, dtype=np.int32)
    _check(lib().crsdr_beam_adapt(_p(aw.view(np.float32), C.c_float), _p(info, C.c_float), _p(stat, C.c_int32), _p(a.view(np.float32), C.c_float), nrows, nd, R, int(ref_row),
                                  _p(w.view(np.float32), C.c_float), int(w.shape[0]), C.byref(desc), MEM_HOST))
    return aw, info, int(stat[0])


def beam_adapt_device(aw_ptr: int, ainfo_ptr: int, astat_ptr: int, chi_ptr: int, nrows, nd, R, ref_row, weights, desc: "BeamAdaptDesc"):
    """crsdr_beam_adapt with CRSDR_MEM_DEVICE: aw, ainfo, astat (any but not all may be 0) and chi on the device, the weights on the host."""
    cast = lambda p, t: C.cast(C.c_void_p(int(p) or None), C.POINTER(t))
    w = np.ascontiguousarray(weights, dtype=np.complex64)
    _check(lib().crsdr_beam_adapt(cast(aw_ptr, C.c_float), cast(ainfo_ptr, C.c_float), cast(astat_ptr, C.c_int32), cast(chi_ptr, C.c_float), int(nrows), int(nd), int(R),
                                  int(ref_row), _p(w.view(np.float32), C.c_float), int(w.shape[0]), C.byref(desc), MEM_DEVICE))


def beam_fuse(bdet, bcount, nd, R):
    """crsdr_beam_fuse on ONE line: bdet [nbeams][K][8] float32, bcount [nbeams] int32 -> (fused [K][8] float32 = lag, doppler, power,
    snr, noise, dlag, ddop, beam; nfused).  The engine's fusion on one line, bit for bit."""
    t = np.ascontiguousarray(bdet, dtype=np.float32)
    nb, K, _ = t.shape
    n = np.ascontiguousarray(bcount, dtype=np.int32).reshape(nb)
    out, nf = np.zeros((K, 8), dtype=np.float32), np.zeros(1, dtype=np.int32)
    _check(lib().crsdr_beam_fuse(_p(out, C.c_float), _p(nf, C.c_int32), _p(t, C.c_float), _p(n, C.c_int32), nb, K, int(nd), int(R), MEM_HOST))
    return out, int(nf[0])


def beam_fuse_device(fused_ptr: int, nfused_ptr: int, bdet_ptr: int, bcount_ptr: int, nbeams, K, nd, R):
    """crsdr_beam_fuse with CRSDR_MEM_DEVICE: every pointer on the device (fused or nfused, not both, may be 0)."""
    cast = lambda p, t: C.cast(C.c_void_p(int(p) or None), C.POINTER(t))
    _check(lib().crsdr_beam_fuse(cast(fused_ptr, C.c_float), cast(nfused_ptr, C.c_int32), cast(bdet_ptr, C.c_float), cast(bcount_ptr, C.c_int32), int(nbeams), int(K),
                                 int(nd), int(R), MEM_DEVICE))


def track_desc(max_tracks, m=3, n=5, gate=9.0, sigma_r=0.5, sigma_f=0.5, p0_g=1.0, q_r=1e-3, q_f=1e-3, q_g=1e-4, coupling=0.0, tent_miss=2, conf_miss=4,
               source=TRACK_SRC_ARRAY):
    return TrackDesc(int(max_tracks), int(source), float(sigma_r), float(sigma_f), float(gate), float(p0_g), float(q_r), float(q_f), float(q_g), float(coupling),
                     int(m), int(n), int(tent_miss), int(conf_miss))


def track_state_bytes(desc) -> int:
    """crsdr_track_state_bytes: the size of track()'s state buffer, a 16-byte header and 128 bytes per slot."""
    n = C.c_size_t(0)
    _check(lib().crsdr_track_state_bytes(C.byref(desc), C.byref(n)))
    return int(n.value)


def track(det, count, nd, R, desc, aux=None, state=None):
    """crsdr_track on nlines lines: det [nlines][K][8] float32, count [nlines] int32, aux [nlines][K][2] float32 or None -> (trk
    [nlines][T][16] float32 = id, status, r, f, g, sqrt(P00), sqrt(P11), age, hits, misses, slot, d2, power, snr, aux0, aux1; ntrk
    [nlines][4] int32 = live, confirmed, initiated, dropped; state).  state: the uint8 array an earlier call returned, or None for the
    empty table; it is not changed, the state behind the last line is returned.  The engine's tracker (Caf.set_track), bit for bit."""
    t = np.ascontiguousarray(det, dtype=np.float32)
    L, K, _ = t.shape
    n = np.ascontiguousarray(count, dtype=np.int32).reshape(L)
    a = None if aux is None else np.ascontiguousarray(aux, dtype=np.float32).reshape(L, K, 2)
    nbytes = track_state_bytes(desc)
    s = np.zeros(nbytes // 8, dtype=np.float64).view(np.uint8) if state is None else np.array(state, dtype=np.uint8).reshape(nbytes).copy()
    out, nout = np.zeros((L, int(desc.max_tracks), 16), dtype=np.float32), np.zeros((L, 4), dtype=np.int32)
    _check(lib().crsdr_track(_p(out, C.c_float), _p(nout, C.c_int32), s.ctypes.data_as(C.c_void_p), _p(t, C.c_float), _p(n, C.c_int32), _p(a, C.c_float), L, K, int(nd),
                             int(R), C.byref(desc), MEM_HOST))
    return out, nout, s


def track_device(trk_ptr: int, ntrk_ptr: int, state_ptr: int, det_ptr: int, count_ptr: int, aux_ptr: int, nlines, K, nd, R, desc):
    """crsdr_track with CRSDR_MEM_DEVICE: every pointer on the device (trk or ntrk, not both, and aux may be 0)."""
    cast = lambda p, t: C.cast(C.c_void_p(int(p) or None), C.POINTER(t))
    _check(lib().crsdr_track(cast(trk_ptr, C.c_float), cast(ntrk_ptr, C.c_int32), C.c_void_p(int(state_ptr) or None), cast(det_ptr, C.c_float), cast(count_ptr, C.c_int32),
                             cast(aux_ptr, C.c_float), int(nlines), int(K), int(nd), int(R), C.byref(desc), MEM_DEVICE))


def integrate_desc(forget, coupling=0.0, what=INTEGRATE_ARRAY):
    return IntegrateDesc(int(what), 0, float(forget), float(coupling))


def map_integrate_state_bytes(nmaps, nd, R) -> int:
    """crsdr_map_integrate_state_bytes: the size of map_integrate()'s state buffer, a 16-byte header (int64 m, int64 0) and nmaps nd R
    doubles."""
    n = C.c_size_t(0)
    _check(lib().crsdr_map_integrate_state_bytes(int(nmaps), int(nd), int(R), C.byref(n)))
    return int(n.value)


def map_integrate(maps, desc, state=None):
    """crsdr_map_integrate on nlines lines: maps [nlines][nmaps][nd][R] float32 (or [nlines][nd][R]: one map a line) -> (imap of the same
    shape, state).  state: the uint8 array an earlier call returned, or None for the empty state; it is not changed, the state behind
    the last line is returned.  The engine's integration (Caf.set_integrate), bit for bit."""
    m = np.ascontiguousarray(maps, dtype=np.float32)
    L, nmaps, nd, R = m.shape if m.ndim == 4 else (m.shape[0], 1) + m.shape[1:]
    nbytes = map_integrate_state_bytes(nmaps, nd, R)
    s = np.zeros(nbytes // 8, dtype=np.float64).view(np.uint8) if state is None else np.array(state, dtype=np.uint8).reshape(nbytes).copy()
    out = np.zeros(m.shape, dtype=np.float32)
    _check(lib().crsdr_map_integrate(_p(out, C.c_float), s.ctypes.data_as(C.c_void_p), _p(m, C.c_float), L, nmaps, nd, R, C.byref(desc), MEM_HOST))
    return out, s


def map_integrate_device(imap_ptr: int, state_ptr: int, maps_ptr: int, nlines, nmaps, nd, R, desc):
    """crsdr_map_integrate with CRSDR_MEM_DEVICE: every pointer on the device."""
    cast = lambda p, t: C.cast(C.c_void_p(int(p) or None), C.POINTER(t))
    _check(lib().crsdr_map_integrate(cast(imap_ptr, C.c_float), C.c_void_p(int(state_ptr) or None), cast(maps_ptr, C.c_float), int(nlines), int(nmaps), int(nd), int(R),
                                     C.byref(desc), MEM_DEVICE))


def ambiguity_device(chi_ptr: int, map_ptr: int, peak_ptr: int, matrix_ptr: int, nrows, B, seg, nlags, ref_row, window, guard):
    """Same on device memory (any output pointer, not all, may be 0); returns after the kernels finished."""
    cast = lambda p, t: C.cast(C.c_void_p(int(p) or None), C.POINTER(t))
    _check(lib().crsdr_ambiguity(cast(chi_ptr, C.c_float), cast(map_ptr, C.c_float), cast(peak_ptr, C.c_float), cast(matrix_ptr, C.c_int8), int(nrows), int(B),
                                 int(seg), int(nlags), int(ref_row), int(window), int(guard), MEM_DEVICE))


def ambiguity_cancel(matrix, seg, nlags, taps, dopp=0, ref_row=0, window=WINDOW_RECT, guard=0):
    """crsdr_ambiguity_cancel: ambiguity() with the reference's first `taps` delays, each at -dopp .. dopp Doppler bins, projected out of
    every row but ref_row -> (chi, map, peak, coef [nrows][taps (2 dopp + 1)] complex64, cinfo [nrows][2] float32 = residual share,
    status).  The engine (Caf.set_cancel) on one line of one packet, bit for bit."""
    m = np.ascontiguousarray(matrix, dtype=np.int8)
    nrows, B = m.shape
    nd, R, n = max(B // (2 * max(int(seg), 1)), 0), max(int(nlags), 0), max(int(taps) * (2 * int(dopp) + 1), 0)
    chi, mp, pk = np.empty((nrows, nd, R), dtype=np.complex64), np.empty((nd, R), dtype=np.float32), np.empty((nrows + 1, 6), dtype=np.float32)
    coef, cinfo = np.empty((nrows, n), dtype=np.complex64), np.empty((nrows, 2), dtype=np.float32)
    _check(lib().crsdr_ambiguity_cancel(_p(chi.view(np.float32), C.c_float), _p(mp, C.c_float), _p(pk, C.c_float), _p(m, C.c_int8), nrows, B, int(seg), int(nlags),
                                        int(ref_row), int(window), int(guard), MEM_HOST, int(taps), int(dopp), _p(coef.view(np.float32), C.c_float), _p(cinfo, C.c_float)))
    return chi, mp, pk, coef, cinfo


def clean_shapes(nrows, nd, R, n1, K, clean: "CleanDesc"):
    """{name: (shape, dtype)} of one line's outputs of crsdr_ambiguity_clean, in CLEAN_KEYS' order"""
    T, per = int(clean.max_targets), (2 * int(clean.wl) + 1) * (2 * int(clean.wq) + 1)
    c64, f32, i32 = np.complex64, np.float32, np.int32
    return {"chi": ((nrows, nd, R), c64), "map": ((nd, R), f32), "peak": ((nrows + 1, 6), f32), "coef": ((nrows, n1), c64), "cinfo": ((nrows, 2), f32),
            "det": ((nrows + 1, K, 8), f32), "count": ((nrows + 1,), i32), "snap": ((K, nrows), c64), "tgt": ((T, 8), f32), "ntgt": ((1,), i32),
            "tcoef": ((nrows, T, per), c64), "tinfo": ((nrows, 2), f32), "rchi": ((nrows, nd, R), c64), "rmap": ((nd, R), f32), "rdet": ((nrows + 1, K, 8), f32),
            "rcount": ((nrows + 1,), i32), "rsnap": ((K, nrows), c64)}


def ambiguity_clean(matrix, seg, nlags, cancel: "CancelDesc", cfar: "CfarDesc", clean: "CleanDesc", est: "CfarEstDesc | None" = None, ref_row=0, window=WINDOW_RECT,
                    guard=0) -> dict:
    """crsdr_ambiguity_clean: canceller, detector and the second cancellation stage on one packet's matrix [nrows][B] int8 -> dict of
    CLEAN_KEYS.  The engine (Caf.set_cancel, set_cfar, set_clean) on one line of one packet, bit for bit."""
    m = np.ascontiguousarray(matrix, dtype=np.int8)
    nrows, B = m.shape
    nd = B // (2 * int(seg)) if seg > 0 else 1
    shapes = clean_shapes(nrows, max(nd, 1), int(nlags), int(cancel.taps) * (2 * int(cancel.dopp) + 1), int(cfar.max_det), clean)
    # (a descriptor beyond its limits is refused by the call: the arrays only have to exist)
    out = {k: np.zeros(sh if all(0 < x < 2 ** 20 for x in sh) else (1,), dtype=dt) for k, (sh, dt) in shapes.items()}
    io = CleanOut(*[out[k].ctypes.data for k in CLEAN_KEYS])
    _check(lib().crsdr_ambiguity_clean(C.byref(io), _p(m, C.c_int8), nrows, B, int(seg), int(nlags), int(ref_row), int(window), int(guard), 0, C.byref(cancel), C.byref(cfar),
                                       None if est is None else C.byref(est), C.byref(clean)))
    return out


def ambiguity_clean_device(ptrs: dict, matrix_ptr: int, nrows, B, seg, nlags, ref_row, window, guard, cancel, cfar, clean, est=None):
    """The same on device pointers (ptrs: CLEAN_KEYS -> address, missing or 0: not asked for)."""
    io = CleanOut(*[int(ptrs.get(k) or 0) or None for k in CLEAN_KEYS])
    _check(lib().crsdr_ambiguity_clean(C.byref(io), C.cast(C.c_void_p(int(matrix_ptr)), C.POINTER(C.c_int8)), int(nrows), int(B), int(seg), int(nlags), int(ref_row),
                                       int(window), int(guard), 1, C.byref(cancel), C.byref(cfar), None if est is None else C.byref(est), C.byref(clean)))


def ambiguity_cancel_device(chi_ptr: int, map_ptr: int, peak_ptr: int, matrix_ptr: int, nrows, B, seg, nlags, ref_row, window, guard, taps, dopp, coef_ptr: int,
                            cinfo_ptr: int):
    """Same on device memory (any output pointer, not all, may be 0); returns after the kernels finished."""
    cast = lambda p, t: C.cast(C.c_void_p(int(p) or None), C.POINTER(t))
    _check(lib().crsdr_ambiguity_cancel(cast(chi_ptr, C.c_float), cast(map_ptr, C.c_float), cast(peak_ptr, C.c_float), cast(matrix_ptr, C.c_int8), int(nrows), int(B),
                                        int(seg), int(nlags), int(ref_row), int(window), int(guard), MEM_DEVICE, int(taps), int(dopp), cast(coef_ptr, C.c_float),
                                        cast(cinfo_ptr, C.c_float)))


def subband_beamform(matrix, weights, nfft, first=0, nbands=1, width=1, window=WINDOW_RECT):
    """crsdr_subband_beamform: out [nbands][nbeams][J][width] complex64 = weights [nbands][nbeams][nrows - 1] applied to the band
    spectra of the signal rows of matrix [nrows][B] int8 (J = B / (2 nfft) segments; c_w sum_c u[c - 1] X_c, no conjugate): the batched
    engine's band beam arithmetic on one matrix."""
    m = np.ascontiguousarray(matrix, dtype=np.int8)
    w = np.ascontiguousarray(weights, dtype=np.complex64)
    nrows, B = m.shape
    if w.ndim != 3 or w.shape[0] != nbands or w.shape[2] != nrows - 1:
        raise ValueError("weights must be [nbands][nbeams][nrows - 1]")
    out = np.empty((w.shape[0], w.shape[1], B // (2 * int(nfft)) if nfft > 0 else 0, max(int(width), 0)), dtype=np.complex64)
    _check(lib().crsdr_subband_beamform(_p(out.view(np.float32), C.c_float), _p(m, C.c_int8), nrows, B, int(nfft), int(first), int(nbands), int(width),
                                        int(window), _p(w.view(np.float32), C.c_float), w.shape[1], MEM_HOST))
    return out


def subband_beamform_device(out_ptr: int, matrix_ptr: int, nrows, B, nfft, first, nbands, width, window, weights_ptr: int, nbeams):
    """Same on device memory; returns after the kernel finished."""
    cast = lambda p, t: C.cast(C.c_void_p(int(p) or None), C.POINTER(t))
    _check(lib().crsdr_subband_beamform(cast(out_ptr, C.c_float), cast(matrix_ptr, C.c_int8), int(nrows), int(B), int(nfft), int(first), int(nbands),
                                        int(width), int(window), cast(weights_ptr, C.c_float), int(nbeams), MEM_DEVICE))


def assemble_slabs(packets_ptr: int, packet_stride: int, nrows: int, B: int, recv_ptr: int, nsrc: int, nblocks: int, stream: int | None = None):
    """crsdr_assemble_slabs: the received slabs [nsrc][nblocks][per][B] into the matrix rows of nblocks packets (device pointers)."""
    _check(lib().crsdr_assemble_slabs(C.c_void_p(int(packets_ptr)), int(packet_stride), int(nrows), int(B), C.c_void_p(int(recv_ptr)),
                                      int(nsrc), int(nblocks), C.c_void_p(stream or 0)))


# ---- exchange slots + the RCCL exchange --------------------------------------------------

def exchange_geometry(nrows: int, B: int, nranks: int) -> dict:
    """crsdr_exchange_geometry: slot_stride / tail_offset of a rank's send slots and the stride of an assembled scalars block."""
    a, t, s = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    _check(lib().crsdr_exchange_geometry(int(nrows), int(B), int(nranks), C.byref(a), C.byref(t), C.byref(s)))
    return {"slot_stride": a.value, "tail_offset": t.value, "scalars_stride": s.value, "per": (nrows - 1) // nranks}


def rooted_blocks(nblocks: int, nranks: int, rank: int) -> range:
    """crsdr_exchange_rooted_blocks: the blocks of a batch of nblocks that `rank` assembles."""
    f, c = C.c_int(0), C.c_int(0)
    _check(lib().crsdr_exchange_rooted_blocks(int(nblocks), int(nranks), int(rank), C.byref(f), C.byref(c)))
    return range(f.value, f.value + c.value)


def assemble_slots(packets_ptr, packet_stride, scalars_ptr, scalars_stride, nrows, B, recv_ptr, nsrc, nblocks, slot_stride, tail_offset,
                   self_rank=-1, self_ptr=None, stream=None):
    """crsdr_assemble_slots: received slots [nsrc][nblocks][slot_stride] -> matrix rows of nblocks packets + their scalars blocks."""
    _check(lib().crsdr_assemble_slots(C.c_void_p(int(packets_ptr)), int(packet_stride), C.c_void_p(int(scalars_ptr or 0)), int(scalars_stride),
                                      int(nrows), int(B), C.c_void_p(int(recv_ptr or 0)), int(nsrc), int(nblocks), int(slot_stride), int(tail_offset),
                                      int(self_rank), C.c_void_p(int(self_ptr or 0)), C.c_void_p(stream or 0)))


def parse_scalars(block: np.ndarray, nrows: int) -> dict:
    """One assembled scalars block (bytes) -> {lag, mag, frac, phasor} like Plan.fetch."""
    raw = np.ascontiguousarray(block).view(np.uint8)
    n = nrows
    return dict(lag=raw[:4 * n].view(np.int32).copy(), mag=raw[4 * n:8 * n].view(np.float32).copy(),
                frac=raw[8 * n:12 * n].view(np.float32).copy(), phasor=raw[12 * n:20 * n].view(np.complex64).copy())


def exchange_schedule(nranks, rank, nblocks, mode, nrows, B, packet_stride=0):
    """crsdr_exchange_schedule: the point-to-point operations of one batch for `rank`, in issue order (list of dicts)."""
    n = C.c_int(0)
    _check(lib().crsdr_exchange_schedule(int(nranks), int(rank), int(nblocks), int(mode), int(nrows), int(B), int(packet_stride), None, 0, C.byref(n)))
    ops = (XOp * max(1, n.value))()
    _check(lib().crsdr_exchange_schedule(int(nranks), int(rank), int(nblocks), int(mode), int(nrows), int(B), int(packet_stride), ops, n.value, C.byref(n)))
    return [dict(peer=o.peer, is_recv=bool(o.is_recv), buffer=o.buffer, block=o.block, offset=int(o.offset), bytes=int(o.bytes)) for o in ops[: n.value]]


def exchange_unique_id() -> bytes:
    buf = C.create_string_buffer(EXCHANGE_ID_BYTES)
    _check(lib().crsdr_exchange_unique_id(buf))
    return buf.raw


class Exchange:
    """crsdr_exchange: the slot exchange over RCCL under the C ABI (one per rank; every rank passes rank 0's unique id)."""

    def __init__(self, unique_id: bytes, nranks: int, rank: int, device: int = 0):
        h = C.c_void_p()
        idbuf = C.create_string_buffer(bytes(unique_id), EXCHANGE_ID_BYTES)
        _check(lib().crsdr_exchange_create(C.byref(h), idbuf, int(nranks), int(rank), int(device)))
        self._h, self.nranks, self.rank = h, nranks, rank
        self._plan, self._keep = None, []

    def batch(self, mode, send_ptr, recv_ptr, nblocks, packets_ptr, packet_stride, scalars_ptr, scalars_stride, nrows, B, stream=None):
        _check(lib().crsdr_exchange_batch(self._h, int(mode), C.c_void_p(int(send_ptr)), C.c_void_p(int(recv_ptr or 0)), int(nblocks),
                                          C.c_void_p(int(packets_ptr)), int(packet_stride), C.c_void_p(int(scalars_ptr or 0)), int(scalars_stride),
                                          int(nrows), int(B), C.c_void_p(stream or 0)))

    # ---- a sharded plan and its exchange as one engine (crsdr_exchange_bind_plan / _submit_batch / _fetch_rooted) ----
    def bind_plan(self, plan, mode=None):
        _check(lib().crsdr_exchange_bind_plan(self._h, plan._h, int(XCHG_STAGED if mode is None else mode)))
        self._plan, self._keep = plan, []

    def submit_batch(self, rows, readcnt=None, lag_mask=None, seq=0, flags=REFNOISE_ENABLED):
        """rows: numpy int8/uint8 [nblocks][nrows][B] on the host (page-locked or not): plan submit + exchange, all enqueued on return."""
        keep = np.ascontiguousarray(rows)
        if keep.ndim == 2:
            keep = keep[None]
        assert keep.shape[1:] == (self._plan.nrows, self._plan.B) and keep.dtype in (np.int8, np.uint8)
        rc_arr = None if readcnt is None else np.ascontiguousarray(readcnt, dtype=np.uint32)
        mk = None if lag_mask is None else np.ascontiguousarray(lag_mask, dtype=np.uint8)
        self._keep.append(keep)                     # stays alive until the batch has been fetched
        _check(lib().crsdr_exchange_submit_batch(self._h, C.c_void_p(keep.ctypes.data), MEM_HOST, keep.shape[0], 0, _p(rc_arr, C.c_uint32),
                                                 _p(mk, C.c_uint8), int(seq), int(flags)))

    def fetch_rooted(self):
        """The oldest outstanding batch: (first, packets [count][packet_bytes] int8, scalars (list of parse_scalars dicts), own_tails dict of
        [nblocks][per] arrays: lag, mag, frac, phasor, readcnt)."""
        p = self._plan
        f, c, nb = C.c_int(), C.c_int(), C.c_int()
        if p is None:                                    # nothing bound: let the library say so
            _check(lib().crsdr_exchange_fetch_rooted(self._h, None, 0, None, 0, None, 0, C.byref(f), C.byref(c), C.byref(nb)))
        T, n, per = p.max_batch, p.nrows, (p.nrows - 1) // self.nranks
        bpr = -(-T // self.nranks)
        pk = np.zeros((bpr, p.packet_bytes), dtype=np.int8)
        sstride = (20 * n + 15) // 16 * 16
        tstride = (24 * per + 15) // 16 * 16
        sc = np.zeros((bpr, sstride), dtype=np.uint8)
        tl = np.zeros((T, tstride), dtype=np.uint8)
        _check(lib().crsdr_exchange_fetch_rooted(self._h, _p(pk, C.c_int8), pk.strides[0], C.c_void_p(sc.ctypes.data), sstride,
                                                 C.c_void_p(tl.ctypes.data), tstride, C.byref(f), C.byref(c), C.byref(nb)))
        if self._keep:
            self._keep.pop(0)
        t = tl[:nb.value]
        tails = dict(lag=t[:, :4 * per].copy().view(np.int32), mag=t[:, 4 * per:8 * per].copy().view(np.float32),
                     frac=t[:, 8 * per:12 * per].copy().view(np.float32), phasor=t[:, 12 * per:20 * per].copy().view(np.complex64),
                     readcnt=t[:, 20 * per:24 * per].copy().view(np.uint32))
        return f.value, pk[:c.value], [parse_scalars(sc[j], n) for j in range(c.value)], tails

    def close(self):
        if getattr(self, "_h", None):
            lib().crsdr_exchange_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- batched plan ---------------------------------------------------------------------------------

class Plan:
    """crsdr_plan: ccoherent + per-row csdrdevice DSP members + cpacketize::write on one GPU."""

    def __init__(self, nrows, blocksize, mode=MODE_FAITHFUL, device=0, row_begin=0, row_count=0, max_batch=1):
        self.nrows, self.B, self.mode, self.max_batch = nrows, blocksize, mode, max_batch
        d = PlanDesc(nrows, blocksize, mode, device, row_begin, row_count, max_batch, 0)
        h = C.c_void_p()
        _check(lib().crsdr_plan_create(C.byref(h), C.byref(d)))
        self._h = h
        self._keep = []
        self.packet_bytes = int(lib().crsdr_plan_packet_bytes(h))
        self.matrix_offset = int(lib().crsdr_plan_matrix_offset(h))

    def set_stream(self, hip_stream: int | None):
        _check(lib().crsdr_plan_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    def submit(self, rows, readcnt=None, lag_mask=None, seq=0, flags=REFNOISE_ENABLED, nblocks=None, block_stride=0):
        """rows: numpy int8/uint8 [nrows][B] (or [nblocks][nrows][B]) on the host, or an int device pointer."""
        rc_arr = None if readcnt is None else np.ascontiguousarray(readcnt, dtype=np.uint32)
        mk = None if lag_mask is None else np.ascontiguousarray(lag_mask, dtype=np.uint8)
        if isinstance(rows, (int, np.integer)):
            ptr, kind = C.c_void_p(int(rows)), MEM_DEVICE
            nb = 1 if nblocks is None else int(nblocks)
        else:
            if rows.dtype not in (np.int8, np.uint8):
                raise TypeError("rows must be int8 (or offset-binary uint8)")
            keep = np.ascontiguousarray(rows)
            if keep.ndim == 2:
                keep = keep[None]
            assert keep.shape[1:] == (self.nrows, self.B)
            nb = keep.shape[0] if nblocks is None else int(nblocks)
            self._keep.append(keep)          # stays alive until the next fetch()/sync()
            ptr, kind = C.c_void_p(keep.ctypes.data), MEM_HOST
        _check(lib().crsdr_plan_submit_batch(self._h, ptr, kind, nb, int(block_stride), _p(rc_arr, C.c_uint32),
                                             _p(mk, C.c_uint8), int(seq), int(flags)))

    def fetch(self, want_packet=True, block=-1):
        n = self.nrows
        lag = np.zeros(n, dtype=np.int32)
        mag = np.zeros(n, dtype=np.float32)
        frac = np.zeros(n, dtype=np.float32)
        ph = np.zeros(2 * n, dtype=np.float32)
        pkt = np.zeros(self.packet_bytes, dtype=np.int8) if want_packet else None
        _check(lib().crsdr_plan_fetch_block(self._h, int(block), _p(lag, C.c_int32), _p(mag, C.c_float), _p(frac, C.c_float),
                                            _p(ph, C.c_float), _p(pkt, C.c_int8)))
        if block == -1:
            self._keep.clear()
        return dict(lag=lag, mag=mag, frac=frac, phasor=ph.view(np.complex64), packet=pkt,
                    matrix=None if pkt is None else pkt[self.matrix_offset:].reshape(self.nrows, self.B))

    def fetch_batch_async(self, lag=None, mag=None, frac=None, phasor=None, packets=None, host_packet_stride=0):
        """crsdr_plan_fetch_batch_async: numpy views of page-locked memory (PinnedArray.array) or None"""
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        _check(lib().crsdr_plan_fetch_batch_async(self._h, ptr(lag), ptr(mag), ptr(frac), ptr(phasor), ptr(packets), int(host_packet_stride)))

    def fetch_wait(self):
        _check(lib().crsdr_plan_fetch_wait(self._h))

    def block(self, rows, **kw):
        self.submit(rows, **kw)
        return self.fetch()

    def sync(self):
        _check(lib().crsdr_plan_sync(self._h))
        self._keep.clear()

    def reset(self):
        _check(lib().crsdr_plan_reset(self._h))

    def device_buffers(self):
        ptrs = [C.c_void_p() for _ in range(5)]
        _check(lib().crsdr_plan_device_buffers(self._h, *[C.byref(p) for p in ptrs]))
        return dict(zip(("packet", "lag", "mag", "frac", "phasor"), [p.value for p in ptrs]))

    def bind_packet(self, device_ptr: int | None, packet_stride: int = 0):
        _check(lib().crsdr_plan_bind_packet(self._h, C.c_void_p(device_ptr or 0), int(packet_stride)))

    def bind_slab(self, device_ptr: int | None, slab_stride: int = 0, hdr_first: int = 0, hdr_count: int = 0):
        """Slab output for sharded plans (crsdr_plan_bind_slab); None returns to packet output."""
        _check(lib().crsdr_plan_bind_slab(self._h, C.c_void_p(device_ptr or 0), int(slab_stride), int(hdr_first), int(hdr_count)))

    def set_frac_apply(self, enable=True, gain=1.0, frac_override=None):
        """crsdr_plan_set_frac_apply: fractional-delay correction of the matrix rows (long-block plans, digital mode)."""
        ov = None if frac_override is None else np.ascontiguousarray(frac_override, dtype=np.float32)
        # enable: False / 0 off, True / 1 on, 2 on without the second work area (the pass repeats its first stage)
        _check(lib().crsdr_plan_set_frac_apply(self._h, int(enable), C.c_float(gain), _p(ov, C.c_float)))

    def set_refcancel(self, taps):
        """crsdr_plan_set_refcancel: the reference-noise canceller with `taps` taps (1, 3, 5, 7, 9); 0 / False turns it off."""
        _check(lib().crsdr_plan_set_refcancel(self._h, int(taps)))
        self.refcancel_taps = int(taps)

    def fetch_refcancel(self, block=-1):
        """crsdr_plan_fetch_refcancel: dict(coef [nrows][taps] complex64, residual [nrows], status [nrows]) of a block of the last batch."""
        n, taps = self.nrows, max(getattr(self, "refcancel_taps", 0), 1)
        coef = np.zeros((n, taps), dtype=np.complex64)
        res, st = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32)
        _check(lib().crsdr_plan_fetch_refcancel(self._h, int(block), _p(coef.view(np.float32), C.c_float), _p(res, C.c_float), _p(st, C.c_int32)))
        return dict(coef=coef, residual=res, status=st)

    def refcancel_buffers(self):
        ptrs = [C.c_void_p() for _ in range(3)]
        taps = C.c_int(0)
        _check(lib().crsdr_plan_refcancel_buffers(self._h, *[C.byref(p) for p in ptrs], C.byref(taps)))
        return dict(zip(("coef", "residual", "status"), [p.value for p in ptrs]), taps=taps.value)

    def bind_slab_ex(self, device_ptr: int | None, slab_stride: int = 0, hdr_first: int = 0, hdr_count: int = 0, tail_offset: int = 0):
        """crsdr_plan_bind_slab_ex: slab output with the per-row {lag, mag, frac, phasor} tail behind the rows of every slot."""
        _check(lib().crsdr_plan_bind_slab_ex(self._h, C.c_void_p(device_ptr or 0), int(slab_stride), int(hdr_first), int(hdr_count), int(tail_offset)))

    @property
    def packet_stride(self) -> int:
        return int(lib().crsdr_plan_packet_stride(self._h))

    def last_elapsed_ms(self) -> float:
        ms = C.c_float(0)
        _check(lib().crsdr_plan_last_elapsed_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def enable_profiling(self, slots: int, kernel_mask: int = 0xF):
        """kernel_mask: bit KERNEL_*; 1 << 31 adds whole-submit start/stop events"""
        _check(lib().crsdr_plan_enable_profiling(self._h, int(slots), int(kernel_mask)))

    def kernel_times_ms(self, which: int, capacity: int = 4096) -> np.ndarray:
        out = np.zeros(capacity, dtype=np.float32)
        n = C.c_int(0)
        _check(lib().crsdr_plan_kernel_times(self._h, int(which), _p(out, C.c_float), capacity, C.byref(n)))
        return out[: n.value].copy()

    def close(self):
        if getattr(self, "_h", None):
            lib().crsdr_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Doa:
    """crsdr_doa: covariance -> noise subspace -> 2-D MUSIC scan + peak for a batch of device-resident packets, one estimate per
    `frames` consecutive packets.  submit* only enqueue; fetch() waits and returns numpy arrays."""

    def __init__(self, nrows, blocksize, k, d, mx, my, ncx=100, ncy=100, max_batch=1, frames=1, flags=0, device=0):
        desc = DoaDesc(int(nrows), int(blocksize), int(device), int(max_batch), int(frames), int(k), int(mx), int(my), int(ncx), int(ncy),
                       float(d), int(flags))
        h = C.c_void_p()
        _check(lib().crsdr_doa_create(C.byref(h), C.byref(desc)))
        self._h = h
        self.nrows, self.B, self.m, self.k, self.ncx, self.ncy = int(nrows), int(blocksize), int(nrows) - 1, int(k), int(ncx), int(ncy)
        self.max_batch, self.frames, self.flags = max(1, int(max_batch)), max(1, int(frames)), int(flags)
        self.d, self._sub = float(d), (int(mx), int(my))                            # _sub: set_smoothing's sub-array
        self.npeaks, self.nbeams = 0, 0
        self.mx, self.my, self.ms, self.order = int(mx), int(my), self.m, None      # ms: the subspace's size; order: (kmin, kmax)
        self.nbands = 0                                                             # set_subbands: bands per estimate (0: off)
        self.band_shape, self.nbandbeams = None, 0                                  # set_subbands: (J, width); set_subband_beams: slots
        self.esprit = ESPRIT_OFF                                                    # set_esprit: the mode

    def _last(self):
        nest, launches = C.c_int(0), C.c_int(0)
        _check(lib().crsdr_doa_last_submit(self._h, C.byref(nest), C.byref(launches)))
        return nest.value, launches.value

    def submit(self, packets_ptr: int, packet_stride: int, matrix_offset: int, nblocks: int, stream: int | None = None):
        """nblocks packets on the device: packet t at packets_ptr + t * packet_stride, its matrix at + matrix_offset."""
        _check(lib().crsdr_doa_submit(self._h, C.c_void_p(int(packets_ptr)), int(packet_stride), int(matrix_offset), int(nblocks),
                                      C.c_void_p(stream or 0)))

    def submit_plan(self, plan: "Plan"):
        """The plan's last submitted batch, where its packets are, on the plan's stream."""
        _check(lib().crsdr_doa_submit_plan(self._h, plan._h))

    def fetch(self, spectrum=None, rxx=None) -> dict:
        """Waits for the last submit.  peak [nest][2] (cx, cy), peak_value [nest], sv [nest][m], status [nest]; pm [nest][ncx][ncy] and
        rxx [nest][m][m] complex64 when the object keeps them (spectrum / rxx: override, e.g. False to skip the copy)."""
        n = self._last()[0]
        want_pm = bool(self.flags & DOA_KEEP_SPECTRUM) if spectrum is None else bool(spectrum)
        want_rxx = bool(self.flags & DOA_KEEP_RXX) if rxx is None else bool(rxx)
        peak, val = np.zeros((n, 2), dtype=np.int32), np.zeros(n, dtype=np.float32)
        sv, status = np.zeros((n, self.ms), dtype=np.float32), np.zeros(n, dtype=np.int32)
        if self.esprit == ESPRIT_ONLY:                   # no scan ran: there is no peak, peak_value or pm to ask for
            peak, val, want_pm = None, None, False
        pm = np.zeros((n, self.ncx, self.ncy), dtype=np.float32) if want_pm else None
        r = np.zeros((n, self.m, self.m), dtype=np.complex64) if want_rxx else None
        _check(lib().crsdr_doa_fetch(self._h, _p(peak, C.c_int32), _p(val, C.c_float), _p(sv, C.c_float), _p(status, C.c_int32),
                                     _p(pm, C.c_float), _p(None if r is None else r.view(np.float32), C.c_float)))
        out = {"peak": peak, "peak_value": val, "sv": sv, "status": status} if peak is not None else {"sv": sv, "status": status}
        if pm is not None:
            out["pm"] = pm
        if r is not None:
            out["rxx"] = r
        return out

    def fetch_peaks(self) -> np.ndarray:
        """Only the directions: peak [nest][2]."""
        peak = np.zeros((self._last()[0], 2), dtype=np.int32)
        _check(lib().crsdr_doa_fetch(self._h, _p(peak, C.c_int32), None, None, None, None, None))
        return peak

    def device_buffers(self) -> dict:
        ptrs = [C.c_void_p() for _ in range(5)]
        _check(lib().crsdr_doa_device_buffers(self._h, *[C.byref(p) for p in ptrs]))
        return dict(zip(("peak", "peak_value", "sv", "vec", "pm"), [p.value for p in ptrs]))

    def set_peaks(self, count: int, radius: int = 1):
        """crsdr_doa_set_peaks: from the next submit on, the `count` strongest local maxima of each spectrum within a
        (2 radius + 1)^2 window (count = 0: off).  Waits for the device if a submit was made."""
        _check(lib().crsdr_doa_set_peaks(self._h, int(count), int(radius)))
        self.npeaks = int(count)

    def fetch_directions(self) -> dict:
        """Waits for the last submit.  found [nest], peaks [nest][count][2] (cx, cy), values [nest][count]; slots from found on hold
        (-1, -1) and -1."""
        n, c = self._last()[0], self.npeaks
        found, peaks, values = np.zeros(n, dtype=np.int32), np.zeros((n, c, 2), dtype=np.int32), np.zeros((n, c), dtype=np.float32)
        _check(lib().crsdr_doa_fetch_directions(self._h, _p(found, C.c_int32), _p(peaks, C.c_int32), _p(values, C.c_float)))
        return {"found": found, "peaks": peaks, "values": values}

    def direction_buffers(self) -> dict:
        ptrs = [C.c_void_p() for _ in range(3)]
        _check(lib().crsdr_doa_direction_buffers(self._h, *[C.byref(p) for p in ptrs]))
        return dict(zip(("found", "peaks", "values"), [p.value for p in ptrs]))

    def set_beams(self, mode: int, loading: float = 1e-2, fixed_angles=None):
        """crsdr_doa_set_beams: from the next submit on, weights, power and one IQ stream per direction (BEAM_CONVENTIONAL / BEAM_MVDR;
        BEAM_OFF frees them).  fixed_angles [n][2] (alpha, beta) in radians: those directions for every estimate; None: the estimate's
        own (set_peaks' count of them, or the peak).  Waits for the device if a submit was made."""
        fa = None if fixed_angles is None else np.ascontiguousarray(fixed_angles, dtype=np.float32).reshape(-1, 2)
        _check(lib().crsdr_doa_set_beams(self._h, int(mode), C.c_float(loading), 0 if fa is None else fa.shape[0], _p(fa, C.c_float)))
        self.nbeams = self.beam_buffers()["nbeams"]

    def fetch_beams(self, weights=True, power=True, beams=True) -> dict:
        """Waits for the last submit.  weights [nest][nbeams][m] complex64, power [nest][nbeams], beams [nblocks][nbeams][B / 2]
        complex64 (each only if asked for)."""
        n, nb = self._last()[0], self.nbeams
        w = np.zeros((n, nb, self.m), dtype=np.complex64) if weights else None
        pw = np.zeros((n, nb), dtype=np.float32) if power else None
        y = np.zeros((n * self.frames, nb, self.B // 2), dtype=np.complex64) if beams else None
        _check(lib().crsdr_doa_fetch_beams(self._h, _p(None if w is None else w.view(np.float32), C.c_float), _p(pw, C.c_float),
                                           _p(None if y is None else y.view(np.float32), C.c_float)))
        return {k: v for k, v in (("weights", w), ("power", pw), ("beams", y)) if v is not None}

    def beam_buffers(self) -> dict:
        ptrs, nb = [C.c_void_p() for _ in range(3)], C.c_int(0)
        _check(lib().crsdr_doa_beam_buffers(self._h, *[C.byref(p) for p in ptrs], C.byref(nb)))
        return dict(zip(("weights", "power", "beams"), [p.value for p in ptrs]), nbeams=nb.value)

    def fetch_subspace(self) -> np.ndarray:
        """vec [nest][m][m] complex64 of the last submit (column r of vec[e] = the singular vector of sv[e][r])."""
        vec = np.zeros((self._last()[0], self.ms, self.ms), dtype=np.complex64)
        _check(lib().crsdr_doa_fetch_subspace(self._h, _p(vec.view(np.float32), C.c_float)))
        return vec

    def set_smoothing(self, sx: int, sy: int, flags: int = 0):
        """crsdr_doa_set_smoothing: from the next submit on, the covariance averaged over its sx x sy sub-arrays (SMOOTH_FB: and with its
        backward image) feeds the subspace; sv and vec then have ms = sx * sy entries.  (mx, my) with flags 0: off.  Waits for the
        device if a submit was made, and discards that submit's results."""
        _check(lib().crsdr_doa_set_smoothing(self._h, int(sx), int(sy), int(flags)))
        self.ms, self._sub = int(sx) * int(sy), (int(sx), int(sy))

    def fetch_smoothed(self) -> np.ndarray:
        """rs [nest][ms][ms] complex64 of the last submit."""
        rs = np.zeros((self._last()[0], self.ms, self.ms), dtype=np.complex64)
        _check(lib().crsdr_doa_fetch_smoothed(self._h, _p(rs.view(np.float32), C.c_float)))
        return rs

    def set_augment(self, vx: int, vy: int = 0, mask=0):
        """crsdr_doa_set_augment: from the next submit on, the covariance of the filled vx x vy virtual array, rebuilt from the per-lag
        averages over the elements of `mask` (mask_bits; 0: all), feeds the subspace; sv and vec then have vx * vy entries.  vx = 0: off.
        Waits for the device if a submit was made, and discards that submit's results."""
        _check(lib().crsdr_doa_set_augment(self._h, int(vx), int(vy), mask_bits(mask)))
        if vx:
            self.ms, self._sub = int(vx) * int(vy), (int(vx), int(vy))
        else:
            self.ms, self._sub = self.m, (self.mx, self.my)

    def fetch_augmented(self) -> np.ndarray:
        """ra [nest][mv][mv] complex64 of the last submit."""
        ra = np.zeros((self._last()[0], self.ms, self.ms), dtype=np.complex64)
        _check(lib().crsdr_doa_fetch_augmented(self._h, _p(ra.view(np.float32), C.c_float)))
        return ra

    def augment_buffers(self) -> dict:
        p, vx, vy = C.c_void_p(), C.c_int(0), C.c_int(0)
        _check(lib().crsdr_doa_augment_buffers(self._h, C.byref(p), C.byref(vx), C.byref(vy)))
        return {"ra": p.value, "vx": vx.value, "vy": vy.value}

    def set_order(self, criterion: int, kmin: int = 1, kmax: int | None = None, limit_directions: bool = False):
        """crsdr_doa_set_order: from the next submit on, every estimate's source count k_e (ORDER_MDL / ORDER_AIC over kmin .. kmax,
        kmax = ms - 1 by default) replaces k in its scan; limit_directions: set_peaks reports at most k_e.  ORDER_OFF: off."""
        kmax = self.ms - 1 if kmax is None else int(kmax)
        _check(lib().crsdr_doa_set_order(self._h, int(criterion), int(kmin), kmax, int(bool(limit_directions))))
        self.order = (int(kmin), kmax) if criterion != ORDER_OFF else None

    def fetch_order(self) -> dict:
        """Waits for the last submit.  k [nest], criterion [nest][kmax - kmin + 1]."""
        n = self._last()[0]
        nc = self.order[1] - self.order[0] + 1 if self.order else 0
        k, crit = np.zeros(n, dtype=np.int32), np.zeros((n, nc), dtype=np.float32)
        _check(lib().crsdr_doa_fetch_order(self._h, _p(k, C.c_int32), _p(crit, C.c_float)))
        return {"k": k, "criterion": crit}

    def order_buffers(self) -> dict:
        ptrs = [C.c_void_p() for _ in range(2)]
        _check(lib().crsdr_doa_order_buffers(self._h, *[C.byref(p) for p in ptrs]))
        return dict(zip(("k", "criterion"), [p.value for p in ptrs]))

    def set_subbands(self, nfft: int, first: int = 0, nbands: int = 1, width: int = 1, window: int = WINDOW_RECT):
        """crsdr_doa_set_subbands: from the next submit on, one covariance per (estimate, band) of `width` bins of an nfft-point
        transform from bin `first` on (FFT order, wrapping); every fetch then counts nest * nbands entries, estimate e's band i at
        e * nbands + i.  nfft = 0: off.  Only while peaks, beams, smoothing and order are off (set them afterwards; the beams of the
        bands are set_subband_beams).
        Waits for the device if a submit was made, and discards that submit's results."""
        _check(lib().crsdr_doa_set_subbands(self._h, int(nfft), int(first), int(nbands), int(width), int(window)))
        self.nbands = int(nbands) if nfft else 0
        self.band_shape = (self.B // (2 * int(nfft)), int(width)) if nfft else None

    def fetch_subbands(self) -> np.ndarray:
        """Waits for the last submit.  power [nest][nbands] = Re trace(R_band) / m."""
        power = np.zeros((self._last()[0] // self.nbands, self.nbands) if self.nbands else (1, 1), dtype=np.float32)      # (off: the library says so)
        _check(lib().crsdr_doa_fetch_subbands(self._h, _p(power, C.c_float)))
        return power

    def subband_buffers(self) -> dict:
        p = C.c_void_p()
        _check(lib().crsdr_doa_subband_buffers(self._h, C.byref(p)))
        return {"power": p.value}

    def set_subband_beams(self, mode: int, loading: float = 1e-2, fixed_angles=None):
        """crsdr_doa_set_subband_beams: with subbands on, from the next submit on, weights and power per (estimate, band, slot) and one
        narrowband IQ stream per (packet, band, slot): the band's weights applied to the rows' band spectra.  Arguments as set_beams.
        Waits for the device if a submit was made."""
        fa = None if fixed_angles is None else np.ascontiguousarray(fixed_angles, dtype=np.float32).reshape(-1, 2)
        _check(lib().crsdr_doa_set_subband_beams(self._h, int(mode), C.c_float(loading), 0 if fa is None else fa.shape[0], _p(fa, C.c_float)))
        self.nbandbeams = self.subband_beam_buffers()["nbeams"]

    def fetch_subband_beams(self, weights=True, power=True, beams=True) -> dict:
        """Waits for the last submit.  weights [nest * nbands][nbeams][m] complex64, power [nest * nbands][nbeams], beams
        [nblocks][nbands][nbeams][J][width] complex64 (each only if asked for)."""
        n, nb = self._last()[0], self.nbandbeams
        nbands, (J, width) = max(self.nbands, 1), self.band_shape or (0, 0)
        w = np.zeros((n, nb, self.m), dtype=np.complex64) if weights else None
        pw = np.zeros((n, nb), dtype=np.float32) if power else None
        y = np.zeros((n // nbands * self.frames, nbands, nb, J, width), dtype=np.complex64) if beams else None
        _check(lib().crsdr_doa_fetch_subband_beams(self._h, _p(None if w is None else w.view(np.float32), C.c_float), _p(pw, C.c_float),
                                                   _p(None if y is None else y.view(np.float32), C.c_float)))
        return {k: v for k, v in (("weights", w), ("power", pw), ("beams", y)) if v is not None}

    def subband_beam_buffers(self) -> dict:
        ptrs, nb = [C.c_void_p() for _ in range(3)], C.c_int(0)
        _check(lib().crsdr_doa_subband_beam_buffers(self._h, *[C.byref(p) for p in ptrs], C.byref(nb)))
        return dict(zip(("weights", "power", "beams"), [p.value for p in ptrs]), nbeams=nb.value)

    def set_spectrum(self, kind: int, loading: float = 1e-2):
        """crsdr_doa_set_spectrum: from the next submit on the scan computes the Bartlett or the Capon power map (SPECTRUM_BARTLETT,
        SPECTRUM_CAPON with its diagonal loading) in place of the MUSIC pseudo-spectrum (SPECTRUM_MUSIC: back to it), and pm, peak, the
        directions and the beams that follow them work on that map.  Waits for the device if a submit was made; what it left is gone."""
        _check(lib().crsdr_doa_set_spectrum(self._h, int(kind), C.c_float(loading)))

    def set_refine(self, levels: int = 5):
        """crsdr_doa_set_refine: from the next submit on every direction (set_peaks' slots, or the peak) is refined off the grid by
        `levels` levels (1 .. 8) of the fp64 zoom search, and following beams steer there.  0: off.  Waits for the device if a submit
        was made."""
        _check(lib().crsdr_doa_set_refine(self._h, int(levels)))

    def fetch_refined(self) -> dict:
        """Waits for the last submit.  offsets [nest][slots][2] (grid cells, exact), angles [nest][slots][2] (alpha, beta in radians),
        values [nest][slots]; empty slots hold (0, 0), (-1, -1) and -1."""
        n, c = self._last()[0], self.refined_buffers()["slots"]
        off, ang, val = np.zeros((n, c, 2), dtype=np.float32), np.zeros((n, c, 2), dtype=np.float32), np.zeros((n, c), dtype=np.float32)
        _check(lib().crsdr_doa_fetch_refined(self._h, _p(off, C.c_float), _p(ang, C.c_float), _p(val, C.c_float)))
        return {"offsets": off, "angles": ang, "values": val}

    def refined_buffers(self) -> dict:
        ptrs, slots = [C.c_void_p() for _ in range(3)], C.c_int(0)
        _check(lib().crsdr_doa_refined_buffers(self._h, *[C.byref(p) for p in ptrs], C.byref(slots)))
        return dict(zip(("offsets", "angles", "values"), [p.value for p in ptrs]), slots=slots.value)

    def refine2d(self, vec, sv, peaks, kind=SPECTRUM_MUSIC, k=None, loading=1e-2, levels=5) -> dict:
        """crsdr_refine2d with this object's geometry (the sub-arrays' while smoothing is on) on one matrix's vec, sv and directions."""
        M = np.asarray(vec).shape[0]
        sx, sy = (self.mx, self.my) if M == self.m else self._sub
        return refine2d(vec, sv, kind, peaks, self.d, sx, sy, self.ncx, self.ncy, k=self.k if k is None else k, loading=loading, levels=levels)

    def set_esprit(self, mode: int = ESPRIT_BESIDE):
        """crsdr_doa_set_esprit: from the next submit on the k directions of every matrix by 2-D ESPRIT, beside the scan (ESPRIT_BESIDE)
        or in its place (ESPRIT_ONLY: no scan, peak, local peaks or refinement are issued).  ESPRIT_OFF: off.  Waits for the device if a
        submit was made."""
        _check(lib().crsdr_doa_set_esprit(self._h, int(mode)))
        self.esprit = int(mode)

    def fetch_esprit(self, want=None) -> dict:
        """Waits for the last submit.  found, status [nest]; phases [nest][slots][2] float64 (mu, nu); angles [nest][slots][2] (alpha, beta
        in radians); modulus [nest][slots][2]; power, flags [nest][slots]; empty slots hold (0, 0), (-1, -1), (-1, -1), -1 and 0.
        want: the names to copy (a copy each), None: all seven."""
        n, c = self._last()[0], self.esprit_buffers()["slots"]
        shapes = (("found", (n,), np.int32, C.c_int32), ("status", (n,), np.int32, C.c_int32), ("phases", (n, c, 2), np.float64, C.c_double),
                  ("angles", (n, c, 2), np.float32, C.c_float), ("modulus", (n, c, 2), np.float32, C.c_float), ("power", (n, c), np.float32, C.c_float),
                  ("flags", (n, c), np.int32, C.c_int32))
        out = {name: np.zeros(shape, dtype=dt) if want is None or name in want else None for name, shape, dt, _ in shapes}
        _check(lib().crsdr_doa_fetch_esprit(self._h, *[_p(out[name], ct) for name, _, _, ct in shapes]))
        return {name: a for name, a in out.items() if a is not None}

    def esprit_buffers(self) -> dict:
        ptrs, slots = [C.c_void_p() for _ in range(7)], C.c_int(0)
        _check(lib().crsdr_doa_esprit_buffers(self._h, *[C.byref(p) for p in ptrs], C.byref(slots)))
        return dict(zip(("found", "status", "phases", "angles", "modulus", "power", "flags"), [p.value for p in ptrs]), slots=slots.value)

    def esprit2d(self, vec, sv, k=None) -> dict:
        """crsdr_esprit2d with this object's geometry (the sub-arrays' while smoothing is on) on one matrix's vec and sv."""
        M = np.asarray(vec).shape[0]
        sx, sy = (self.mx, self.my) if M == self.m else self._sub
        return esprit2d(vec, sv, self.k if k is None else k, self.d, sx, sy)

    def last_launches(self) -> int:
        return self._last()[1]

    def close(self):
        if self._h:
            lib().crsdr_doa_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Spectra:
    """crsdr_spectra: per line of `frames` consecutive device-resident packets the Welch auto-spectrum of every row, every row's
    cross-spectrum against row 0 and four alignment figures per row.  submit* only enqueue; fetch() waits and returns numpy arrays."""

    def __init__(self, nrows, blocksize, nfft, overlap=0, window=WINDOW_RECT, band=None, max_batch=1, frames=1, device=0):
        lo, hi = band if band is not None else (-(int(nfft) // 4), int(nfft) // 4)
        desc = SpectraDesc(int(nrows), int(blocksize), int(device), int(max_batch), int(frames), int(nfft), int(overlap), int(window), int(lo), int(hi))
        h = C.c_void_p()
        _check(lib().crsdr_spectra_create(C.byref(h), C.byref(desc)))
        self._h = h
        self.nrows, self.B, self.nfft, self.overlap, self.window, self.band = int(nrows), int(blocksize), int(nfft), int(overlap), int(window), (int(lo), int(hi))
        self.max_batch, self.frames = max(1, int(max_batch)), max(1, int(frames))

    def _last(self):
        nest, launches = C.c_int(0), C.c_int(0)
        _check(lib().crsdr_spectra_last_submit(self._h, C.byref(nest), C.byref(launches)))
        return nest.value, launches.value

    def submit(self, packets_ptr: int, packet_stride: int, matrix_offset: int, nblocks: int, stream: int | None = None):
        """nblocks packets on the device: packet t at packets_ptr + t * packet_stride, its matrix at + matrix_offset."""
        _check(lib().crsdr_spectra_submit(self._h, C.c_void_p(int(packets_ptr)), int(packet_stride), int(matrix_offset), int(nblocks),
                                          C.c_void_p(stream or 0)))

    def submit_plan(self, plan: "Plan"):
        """The plan's last submitted batch, where its packets are, on the plan's stream."""
        _check(lib().crsdr_spectra_submit_plan(self._h, plan._h))

    def fetch(self, psd=True, cross=True, align=True) -> dict:
        """Waits for the last submit.  psd [nest][nrows][nfft], cross [nest][nrows][nfft] complex64, align [nest][nrows][4]."""
        n = self._last()[0]
        p = np.zeros((n, self.nrows, self.nfft), dtype=np.float32) if psd else None
        c = np.zeros((n, self.nrows, self.nfft), dtype=np.complex64) if cross else None
        a = np.zeros((n, self.nrows, 4), dtype=np.float32) if align else None
        _check(lib().crsdr_spectra_fetch(self._h, _p(p, C.c_float), _p(None if c is None else c.view(np.float32), C.c_float), _p(a, C.c_float)))
        return {k: v for k, v in (("psd", p), ("cross", c), ("align", a)) if v is not None}

    def device_buffers(self) -> dict:
        ptrs = [C.c_void_p() for _ in range(3)]
        _check(lib().crsdr_spectra_device_buffers(self._h, *[C.byref(p) for p in ptrs]))
        return dict(zip(("psd", "cross", "align"), [p.value for p in ptrs]))

    def last_launches(self) -> int:
        return self._last()[1]

    def close(self):
        if getattr(self, "_h", None):
            lib().crsdr_spectra_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Caf:
    """crsdr_caf: per line of `frames` consecutive device-resident packets every row's range-Doppler map (cross-ambiguity function)
    against row ref_row, the array map and the peak figures.  submit* only enqueue; fetch() waits and returns numpy arrays."""

    def __init__(self, nrows, blocksize, seg, nlags, ref_row=0, window=WINDOW_RECT, guard=0, max_batch=1, frames=1, device=0):
        desc = CafDesc(int(nrows), int(blocksize), int(device), int(max_batch), int(frames), int(seg), int(nlags), int(ref_row), int(window), int(guard))
        h = C.c_void_p()
        _check(lib().crsdr_caf_create(C.byref(h), C.byref(desc)))
        self._h = h
        self.nrows, self.B, self.seg, self.nlags, self.ref_row, self.window, self.guard = int(nrows), int(blocksize), int(seg), int(nlags), int(ref_row), int(window), int(guard)
        self.max_batch, self.frames = max(1, int(max_batch)), max(1, int(frames))
        self.nd = self.frames * (self.B // (2 * self.seg))

    def _last(self):
        nest, launches = C.c_int(0), C.c_int(0)
        _check(lib().crsdr_caf_last_submit(self._h, C.byref(nest), C.byref(launches)))
        return nest.value, launches.value

    def submit(self, packets_ptr: int, packet_stride: int, matrix_offset: int, nblocks: int, stream: int | None = None):
        """nblocks packets on the device: packet t at packets_ptr + t * packet_stride, its matrix at + matrix_offset."""
        _check(lib().crsdr_caf_submit(self._h, C.c_void_p(int(packets_ptr)), int(packet_stride), int(matrix_offset), int(nblocks), C.c_void_p(stream or 0)))

    def submit_plan(self, plan: "Plan"):
        """The plan's last submitted batch, where its packets are, on the plan's stream."""
        _check(lib().crsdr_caf_submit_plan(self._h, plan._h))

    def fetch(self, chi=True, map=True, peak=True) -> dict:
        """Waits for the last submit.  chi [nest][nrows][nd][nlags] complex64, map [nest][nd][nlags], peak [nest][nrows + 1][6]."""
        n = self._last()[0]
        c = np.zeros((n, self.nrows, self.nd, self.nlags), dtype=np.complex64) if chi else None
        m = np.zeros((n, self.nd, self.nlags), dtype=np.float32) if map else None
        p = np.zeros((n, self.nrows + 1, 6), dtype=np.float32) if peak else None
        _check(lib().crsdr_caf_fetch(self._h, _p(None if c is None else c.view(np.float32), C.c_float), _p(m, C.c_float), _p(p, C.c_float)))
        return {k: v for k, v in (("chi", c), ("map", m), ("peak", p)) if v is not None}

    def device_buffers(self) -> dict:
        ptrs = [C.c_void_p() for _ in range(3)]
        _check(lib().crsdr_caf_device_buffers(self._h, *[C.byref(p) for p in ptrs]))
        return dict(zip(("chi", "map", "peak"), [p.value for p in ptrs]))

    def set_cfar(self, desc: "CfarDesc | None"):
        """crsdr_caf_set_cfar: the CFAR detector behind every submit (None: off).  Between submits."""
        _check(lib().crsdr_caf_set_cfar(self._h, None if desc is None else C.byref(desc)))
        self.max_det = 0 if desc is None else int(desc.max_det)

    def set_cfar_estimator(self, est: "CfarEstDesc | None"):
        """crsdr_caf_set_cfar_estimator: the noise estimate of the detector that is on (None: cell averaging).  Between submits; every
        set_cfar puts it back to cell averaging."""
        _check(lib().crsdr_caf_set_cfar_estimator(self._h, None if est is None else C.byref(est)))

    def fetch_cfar(self, det=True, count=True, snap=True) -> dict:
        """Waits for the last submit.  det [nest][nrows + 1][K][8], count [nest][nrows + 1] int32, snap [nest][K][nrows] complex64."""
        n, K = self._last()[0], max(1, getattr(self, "max_det", 0))
        d = np.zeros((n, self.nrows + 1, K, 8), dtype=np.float32) if det else None
        c = np.zeros((n, self.nrows + 1), dtype=np.int32) if count else None
        s = np.zeros((n, K, self.nrows), dtype=np.complex64) if snap else None
        _check(lib().crsdr_caf_fetch_cfar(self._h, _p(d, C.c_float), _p(c, C.c_int32), _p(None if s is None else s.view(np.float32), C.c_float)))
        return {k: v for k, v in (("det", d), ("count", c), ("snap", s)) if v is not None}

    def cfar_device_buffers(self) -> dict:
        ptrs = [C.c_void_p() for _ in range(3)]
        _check(lib().crsdr_caf_cfar_device_buffers(self._h, *[C.byref(p) for p in ptrs]))
        return dict(zip(("det", "count", "snap"), [p.value for p in ptrs]))

    def set_bearing(self, desc: "BearingDesc | None"):
        """crsdr_caf_set_bearing: a direction per detection of the array map behind every submit (None: off).  Between submits, with the
        detector on."""
        _check(lib().crsdr_caf_set_bearing(self._h, None if desc is None else C.byref(desc)))
        self.grid = None if desc is None else (int(desc.ncx), int(desc.ncy), bool(desc.flags & BEARING_KEEP_SPECTRUM))

    def fetch_bearing(self, dir=True, spec=None) -> dict:
        """Waits for the last submit.  dir [nest][K][8] = cx, cy, T, dx, dy, alpha, beta, status; spec [nest][K][ncx][ncy] (by default
        where it is kept)."""
        n, K = self._last()[0], max(1, getattr(self, "max_det", 0))
        ncx, ncy, kept = getattr(self, "grid", None) or (1, 1, False)
        d = np.zeros((n, K, 8), dtype=np.float32) if dir else None
        s = np.zeros((n, K, ncx, ncy), dtype=np.float32) if (kept if spec is None else spec) else None
        _check(lib().crsdr_caf_fetch_bearing(self._h, _p(d, C.c_float), _p(s, C.c_float)))
        return {k: v for k, v in (("dir", d), ("spec", s)) if v is not None}

    def bearing_device_buffers(self) -> dict:
        ptrs = [C.c_void_p() for _ in range(2)]
        _check(lib().crsdr_caf_bearing_device_buffers(self._h, *[C.byref(p) for p in ptrs]))
        return dict(zip(("dir", "spec"), [p.value for p in ptrs]))

    def set_beams(self, weights, flags=0):
        """crsdr_caf_set_beams: coherent beam maps across the rows behind every submit, weights [nbeams][nrows - 1] complex64 (None:
        off).  Between submits.  With the detector on at this call every beam map is detected on and the lists are fused."""
        desc = None if weights is None else (weights if isinstance(weights, BeamsDesc) else beams_desc(weights, flags))
        _check(lib().crsdr_caf_set_beams(self._h, None if desc is None else C.byref(desc)))
        self.nbeams, self.beams_detect = (0, False) if desc is None else (int(desc.nbeams), getattr(self, "max_det", 0) > 0)

    def fetch_beams(self, bmap=True, lists=None, fused_only=False) -> dict:
        """Waits for the last submit.  bmap [nest][nb][nd][nlags]; with the lists (by default where the detector was on at set_beams)
        bdet [nest][nb][K][8], bcount [nest][nb] int32, fused [nest][K][8] = lag, doppler, power, snr, noise, dlag, ddop, beam, and
        nfused [nest] int32; fused_only leaves bdet and bcount on the device."""
        n, nb, K = self._last()[0], max(1, getattr(self, "nbeams", 0)), max(1, getattr(self, "max_det", 0))
        lists = getattr(self, "beams_detect", False) if lists is None else lists
        m = np.zeros((n, nb, self.nd, self.nlags), dtype=np.float32) if bmap else None
        d = np.zeros((n, nb, K, 8), dtype=np.float32) if lists and not fused_only else None
        c = np.zeros((n, nb), dtype=np.int32) if lists and not fused_only else None
        f = np.zeros((n, K, 8), dtype=np.float32) if lists else None
        nf = np.zeros(n, dtype=np.int32) if lists else None
        _check(lib().crsdr_caf_fetch_beams(self._h, _p(m, C.c_float), _p(d, C.c_float), _p(c, C.c_int32), _p(f, C.c_float), _p(nf, C.c_int32)))
        return {k: v for k, v in (("bmap", m), ("bdet", d), ("bcount", c), ("fused", f), ("nfused", nf)) if v is not None}

    def set_beam_adapt(self, desc: "BeamAdaptDesc | None"):
        """crsdr_caf_set_beam_adapt: per line MVDR weights from the covariance of the line's own training cells in place of the beams'
        weights (None: off).  Between submits, with beams on and the integration and the tracker off; every set_beams turns it off."""
        _check(lib().crsdr_caf_set_beam_adapt(self._h, None if desc is None else C.byref(desc)))

    def fetch_beam_adapt(self, aw=True, ainfo=True, astat=True) -> dict:
        """Waits for the last submit.  aw [nest][nb][nrows - 1] complex64, ainfo [nest][nb][2] = the training cells' mean power through
        the adaptive beam and through the caller's, astat [nest] int32 (0, or the fallback's bits)."""
        n, nb = self._last()[0], max(1, getattr(self, "nbeams", 0))
        w = np.zeros((n, nb, self.nrows - 1), dtype=np.complex64) if aw else None
        i = np.zeros((n, nb, 2), dtype=np.float32) if ainfo else None
        s = np.zeros(n, dtype=np.int32) if astat else None
        _check(lib().crsdr_caf_fetch_beam_adapt(self._h, _p(None if w is None else w.view(np.float32), C.c_float), _p(i, C.c_float), _p(s, C.c_int32)))
        return {k: v for k, v in (("aw", w), ("ainfo", i), ("astat", s)) if v is not None}

    def beam_adapt_device_buffers(self) -> dict:
        ptrs = [C.c_void_p() for _ in range(3)]
        _check(lib().crsdr_caf_beam_adapt_device_buffers(self._h, *[C.byref(p) for p in ptrs]))
        return dict(zip(("aw", "ainfo", "astat"), [p.value for p in ptrs]))

    def beams_device_buffers(self) -> dict:
        ptrs = [C.c_void_p() for _ in range(5)]
        _check(lib().crsdr_caf_beams_device_buffers(self._h, *[C.byref(p) for p in ptrs]))
        return dict(zip(("bmap", "bdet", "bcount", "fused", "nfused"), [p.value for p in ptrs]))

    def set_track(self, desc: "TrackDesc | None"):
        """crsdr_caf_set_track: the tracker behind every submit's lists (None: off); empties its state.  Between submits, with the
        detector on; the fused source with beams detected on."""
        _check(lib().crsdr_caf_set_track(self._h, None if desc is None else C.byref(desc)))
        self.max_tracks = 0 if desc is None else int(desc.max_tracks)

    def track_reset(self):
        """crsdr_caf_track_reset: the empty table, ids from 1."""
        _check(lib().crsdr_caf_track_reset(self._h))

    def fetch_track(self, trk=True, ntrk=True) -> dict:
        """Waits for the last submit.  trk [nest][T][16] as track() lays it out, ntrk [nest][4] int32 = live, confirmed, initiated,
        dropped."""
        n, T = self._last()[0], max(1, getattr(self, "max_tracks", 0))
        t = np.zeros((n, T, 16), dtype=np.float32) if trk else None
        c = np.zeros((n, 4), dtype=np.int32) if ntrk else None
        _check(lib().crsdr_caf_fetch_track(self._h, _p(t, C.c_float), _p(c, C.c_int32)))
        return {k: v for k, v in (("trk", t), ("ntrk", c)) if v is not None}

    def track_device_buffers(self) -> dict:
        ptrs = [C.c_void_p() for _ in range(2)]
        _check(lib().crsdr_caf_track_device_buffers(self._h, *[C.byref(p) for p in ptrs]))
        return dict(zip(("trk", "ntrk"), [p.value for p in ptrs]))

    def set_integrate(self, desc: "IntegrateDesc | None"):
        """crsdr_caf_set_integrate: the maps integrated across lines along the range walk, ahead of the detector (None: off); empties
        its state.  Between submits, with bearings and the tracker off; INTEGRATE_BEAMS with beams on."""
        _check(lib().crsdr_caf_set_integrate(self._h, None if desc is None else C.byref(desc)))
        self.integrate = 0 if desc is None else int(desc.what)

    def integrate_reset(self):
        """crsdr_caf_integrate_reset: the empty state, m = 0."""
        _check(lib().crsdr_caf_integrate_reset(self._h))

    def fetch_integrate(self, imap=None, ibmap=None) -> dict:
        """Waits for the last submit.  imap [nest][nd][nlags], ibmap [nest][nb][nd][nlags]; by default those whose flag is on."""
        n, what, nb = self._last()[0], getattr(self, "integrate", 0), max(1, getattr(self, "nbeams", 0))
        a = np.zeros((n, self.nd, self.nlags), dtype=np.float32) if (what & INTEGRATE_ARRAY if imap is None else imap) else None
        m = np.zeros((n, nb, self.nd, self.nlags), dtype=np.float32) if (what & INTEGRATE_BEAMS if ibmap is None else ibmap) else None
        _check(lib().crsdr_caf_fetch_integrate(self._h, _p(a, C.c_float), _p(m, C.c_float)))
        return {k: v for k, v in (("imap", a), ("ibmap", m)) if v is not None}

    def integrate_device_buffers(self) -> dict:
        ptrs = [C.c_void_p() for _ in range(3)]
        _check(lib().crsdr_caf_integrate_device_buffers(self._h, *[C.byref(p) for p in ptrs]))
        return dict(zip(("imap", "ibmap", "state"), [p.value for p in ptrs]))

    def set_cancel(self, taps: "int | None", dopp: int = 0):
        """crsdr_caf_set_cancel: the canceller in front of every submit's Doppler stage (taps None: off).  Between submits."""
        desc = None if taps is None else CancelDesc(int(taps), int(dopp))
        _check(lib().crsdr_caf_set_cancel(self._h, None if desc is None else C.byref(desc)))
        self.basis = 0 if desc is None else int(taps) * (2 * int(dopp) + 1)

    def fetch_cancel(self, coef=True, cinfo=True) -> dict:
        """Waits for the last submit.  coef [nest][nrows][n] complex64, cinfo [nest][nrows][2] = residual share, status."""
        n, b = self._last()[0] if getattr(self, "basis", 0) else 0, max(1, getattr(self, "basis", 0))
        c = np.zeros((n, self.nrows, b), dtype=np.complex64) if coef else None
        i = np.zeros((n, self.nrows, 2), dtype=np.float32) if cinfo else None
        _check(lib().crsdr_caf_fetch_cancel(self._h, _p(None if c is None else c.view(np.float32), C.c_float), _p(i, C.c_float)))
        return {k: v for k, v in (("coef", c), ("cinfo", i)) if v is not None}

    def cancel_device_buffers(self) -> dict:
        ptrs = [C.c_void_p() for _ in range(2)]
        _check(lib().crsdr_caf_cancel_device_buffers(self._h, *[C.byref(p) for p in ptrs]))
        return dict(zip(("coef", "cinfo"), [p.value for p in ptrs]))

    def set_clean(self, desc: "CleanDesc | None"):
        """crsdr_caf_set_clean: the second cancellation stage behind every submit's detector (None: off).  Between submits, with the
        canceller and the detector on."""
        _check(lib().crsdr_caf_set_clean(self._h, None if desc is None else C.byref(desc)))
        self.clean = None if desc is None else (int(desc.max_targets), (2 * int(desc.wl) + 1) * (2 * int(desc.wq) + 1))

    def fetch_clean(self, **want) -> dict:
        """Waits for the last submit.  tgt [nest][T][8], ntgt [nest], tcoef [nest][nrows][T][per] complex64, tinfo [nest][nrows][2], and
        rchi, rmap, rdet, rcount, rsnap as fetch() and fetch_cfar() lay out chi, map, det, count, snap.  name=False leaves one out."""
        n, K = (self._last()[0] if getattr(self, "clean", None) else 0), max(1, getattr(self, "max_det", 0))
        T, per = getattr(self, "clean", None) or (1, 1)
        c64, f32, i32 = np.complex64, np.float32, np.int32
        spec = (("tgt", (n, T, 8), f32), ("ntgt", (n,), i32), ("tcoef", (n, self.nrows, T, per), c64), ("tinfo", (n, self.nrows, 2), f32),
                ("rchi", (n, self.nrows, self.nd, self.nlags), c64), ("rmap", (n, self.nd, self.nlags), f32), ("rdet", (n, self.nrows + 1, K, 8), f32),
                ("rcount", (n, self.nrows + 1), i32), ("rsnap", (n, K, self.nrows), c64))
        out = {k: np.zeros(sh, dtype=dt) for k, sh, dt in spec if want.get(k, True)}
        args = [None if k not in out else _p(out[k].view(f32) if dt is c64 else out[k], C.c_int32 if dt is i32 else C.c_float) for k, _, dt in spec]
        _check(lib().crsdr_caf_fetch_clean(self._h, *args))
        return out

    def clean_device_buffers(self) -> dict:
        ptrs = [C.c_void_p() for _ in range(9)]
        _check(lib().crsdr_caf_clean_device_buffers(self._h, *[C.byref(p) for p in ptrs]))
        return dict(zip(CLEAN_KEYS[8:], [p.value for p in ptrs]))

    def last_launches(self) -> int:
        return self._last()[1]

    def close(self):
        if getattr(self, "_h", None):
            lib().crsdr_caf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
