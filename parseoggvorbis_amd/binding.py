"""ctypes view of the C-ABI in include/vorbis_synth_hip.h (libvorbis_synth_hip.so).

Plumbing only: POD struct mirrors, the symbol table and a loader that FAILS LOUDLY when the HIP
library is missing.  There is no CPU fallback anywhere in this package.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libvorbis_synth_hip.so")

VSYN_MAX_CHANNELS = 32
VSYN_MAX_POSTS = 65
VSYN_OK, VSYN_ERR_INVALID, VSYN_ERR_NO_DEVICE, VSYN_ERR_HIP, VSYN_ERR_STREAM = 0, 1, 2, 3, 4
VSYN_ST_FLOOR_RANGE, VSYN_ST_FLOOR_VALUE, VSYN_ST_GRANULE, VSYN_ST_PLANE_OVERFLOW, VSYN_ST_BAD_MODE = 1, 2, 4, 8, 16
VSYN_ST_BAD_SEGMENT, VSYN_ST_BAD_VQ = 32, 64
VSYN_ST_WINDOW_FLAGS = 128  # accepted by the reference, refused by the device (include/vorbis_synth_hip.h)
VSYN_SEG_RESET = 1
VSYN_SUBMIT_STAGED = 1
VSYN_SUBMIT_INPUTS_READY = 2
VSYN_SUBMIT_KEEP_PCM = 4
VSYN_SUBMIT_PRE_KERNELS = 8
VSYN_PCM_S16, VSYN_PCM_F32 = 1, 2
VSYN_COND_PEAK, VSYN_COND_PREEMPH = 1, 2
VSYN_PITCH_CENTER = 1
VSYN_FDESC_CENTER = 1
VSYN_SPEC_MEL_POWER, VSYN_SPEC_LOG_MEL, VSYN_SPEC_MEL_DB, VSYN_SPEC_MFCC = 1, 2, 3, 4
VSYN_SPEC_LIN_POWER, VSYN_SPEC_LIN_DB, VSYN_SPEC_STFT = 5, 6, 7  # include/vorbis_synth_hip.h, "linear spectra"
VSYN_SPEC_CHROMA, VSYN_SPEC_TONNETZ = 8, 9  # include/vorbis_synth_hip.h, "chroma"
VSYN_CHROMA_NORM_NONE, VSYN_CHROMA_NORM_L1, VSYN_CHROMA_NORM_L2, VSYN_CHROMA_NORM_MAX = 0, 1, 2, 3
VSYN_CHROMA_BASE_C, VSYN_CHROMA_NO_OCT = 1, 2


class Floor1(C.Structure):
    _fields_ = [("multiplier", C.c_uint32), ("num_posts", C.c_uint32), ("xs", C.POINTER(C.c_uint32))]


class Coupling(C.Structure):
    _fields_ = [("magnitude", C.c_uint16), ("angle", C.c_uint16)]


class Mapping(C.Structure):
    _fields_ = [("num_couplings", C.c_uint32), ("couplings", C.POINTER(Coupling)),
                ("channel_floor", C.POINTER(C.c_uint8))]


class Mode(C.Structure):
    _fields_ = [("block_flag", C.c_uint8), ("mapping", C.c_uint8)]


class Setup(C.Structure):
    _fields_ = [("channels", C.c_uint32), ("blocksize0", C.c_uint32), ("blocksize1", C.c_uint32),
                ("num_floors", C.c_uint32), ("floors", C.POINTER(Floor1)),
                ("num_mappings", C.c_uint32), ("mappings", C.POINTER(Mapping)),
                ("num_modes", C.c_uint32), ("modes", C.POINTER(Mode))]


class Taps(C.Structure):
    _fields_ = [("after_envelope", C.c_void_p), ("pcm_after_mdct", C.c_void_p), ("floor_final", C.c_void_p),
                ("floor_curve", C.c_void_p)]


class FeatureSpec(C.Structure):  # vsyn_feature_spec
    _fields_ = [("kind", C.c_uint32), ("output_dim", C.c_uint32), ("options", C.c_uint32), ("reserved0", C.c_uint32),
                ("upscale_xs_factor", C.c_double), ("scale", C.c_float), ("clip_abs_max", C.c_float),
                ("floor_base_factor", C.c_float), ("reserved1", C.c_uint32)]


class SpectralSpec(C.Structure):  # vsyn_spectral_spec
    _fields_ = [("kind", C.c_uint32), ("options", C.c_uint32), ("n_fft", C.c_uint32), ("hop_length", C.c_uint32),
                ("win_length", C.c_uint32), ("n_mels", C.c_uint32), ("n_mfcc", C.c_uint32), ("power", C.c_uint32),
                ("fmin", C.c_double), ("fmax", C.c_double), ("log_floor", C.c_double), ("amin", C.c_double), ("top_db", C.c_double)]


class SpectralChroma(C.Structure):  # vsyn_spectral_chroma
    _fields_ = [("n_chroma", C.c_uint32), ("norm", C.c_uint32), ("options", C.c_uint32), ("reserved", C.c_uint32),
                ("tuning", C.c_double), ("ctroct", C.c_double), ("octwidth", C.c_double)]


class SpectralPost(C.Structure):  # vsyn_spectral_post
    _fields_ = [("order", C.c_uint32), ("width", C.c_uint32), ("norm", C.c_uint32), ("stats", C.c_uint32), ("std_floor", C.c_double),
                ("mean", C.c_void_p), ("std", C.c_void_p)]


class SpectralPcen(C.Structure):  # vsyn_spectral_pcen
    _fields_ = [("gain", C.c_double), ("bias", C.c_double), ("power", C.c_double), ("time_constant", C.c_double), ("eps", C.c_double),
                ("b", C.c_double), ("scale", C.c_double)]


class SpectralHpss(C.Structure):  # vsyn_spectral_hpss
    _fields_ = [("kh", C.c_uint32), ("kp", C.c_uint32), ("component", C.c_uint32), ("output", C.c_uint32), ("power", C.c_double),
                ("margin_h", C.c_double), ("margin_p", C.c_double)]


class PcmEffect(C.Structure):  # vsyn_pcm_effect
    _fields_ = [("n_fft", C.c_uint32), ("hop_length", C.c_uint32), ("win_length", C.c_uint32), ("reserved", C.c_uint32), ("hpss", SpectralHpss)]


class PcmStretch(C.Structure):  # vsyn_pcm_stretch
    _fields_ = [("n_fft", C.c_uint32), ("hop_length", C.c_uint32), ("win_length", C.c_uint32), ("options", C.c_uint32),
                ("shift_to_hz", C.c_uint32), ("reserved", C.c_uint32)]


VSYN_STRETCH_FIX_LENGTH = 1


class OnsetSpec(C.Structure):  # vsyn_onset_spec
    _fields_ = [("lag", C.c_uint32), ("max_size", C.c_uint32), ("n_fft", C.c_uint32), ("hop_length", C.c_uint32), ("options", C.c_uint32)]


class OnsetPeaks(C.Structure):  # vsyn_onset_peaks
    _fields_ = [("pre_max", C.c_double), ("post_max", C.c_double), ("pre_avg", C.c_double), ("post_avg", C.c_double), ("wait", C.c_double),
                ("delta", C.c_double), ("hop_length", C.c_uint32), ("options", C.c_uint32)]


class TempogramSpec(C.Structure):  # vsyn_tempogram_spec
    _fields_ = [("win_length", C.c_uint32), ("hop_length", C.c_uint32), ("options", C.c_uint32), ("reserved", C.c_uint32),
                ("ac_size", C.c_double)]


class RhythmSpec(C.Structure):  # vsyn_rhythm_spec
    _fields_ = [("output", C.c_uint32), ("reserved", C.c_uint32), ("onset", OnsetSpec), ("peaks", OnsetPeaks), ("tempogram", TempogramSpec)]


class TempoSpec(C.Structure):  # vsyn_tempo_spec
    _fields_ = [("start_bpm", C.c_double), ("std_bpm", C.c_double), ("max_tempo", C.c_double)]


VSYN_BEAT_TRIM = 1


class BeatSpec(C.Structure):  # vsyn_beat_spec, 32 bytes
    _fields_ = [("tightness", C.c_double), ("start_bpm", C.c_double), ("bpm", C.c_double), ("hop_length", C.c_uint32), ("options", C.c_uint32)]


class PcmCond(C.Structure):  # vsyn_pcm_cond
    _fields_ = [("options", C.c_uint32), ("reserved", C.c_uint32), ("preemphasis", C.c_double)]


class PcmTrim(C.Structure):  # vsyn_pcm_trim
    _fields_ = [("frame_length", C.c_uint32), ("hop_length", C.c_uint32), ("top_db", C.c_double)]


class PitchSpec(C.Structure):  # vsyn_pitch_spec
    _fields_ = [("frame_length", C.c_uint32), ("hop_length", C.c_uint32), ("options", C.c_uint32), ("reserved", C.c_uint32),
                ("fmin", C.c_double), ("fmax", C.c_double), ("trough_threshold", C.c_double)]


class PyinSpec(C.Structure):  # vsyn_pyin_spec; threshold_probs points into the caller's float64 array, which must outlive the spec's use
    _fields_ = [("frame_length", C.c_uint32), ("hop_length", C.c_uint32), ("options", C.c_uint32), ("n_thresholds", C.c_uint32),
                ("fmin", C.c_double), ("fmax", C.c_double), ("boltzmann_parameter", C.c_double), ("resolution", C.c_double),
                ("max_transition_rate", C.c_double), ("switch_prob", C.c_double), ("no_trough_prob", C.c_double),
                ("threshold_probs", C.c_void_p)]


class FdescSpec(C.Structure):  # vsyn_fdesc_spec
    _fields_ = [("n_fft", C.c_uint32), ("hop_length", C.c_uint32), ("win_length", C.c_uint32), ("options", C.c_uint32),
                ("roll_percent", C.c_double), ("zcr_threshold", C.c_double), ("amin", C.c_double)]


class CqtSpec(C.Structure):  # vsyn_cqt_spec
    _fields_ = [("n_bins", C.c_uint32), ("bins_per_octave", C.c_uint32), ("hop_length", C.c_uint32), ("options", C.c_uint32),
                ("output", C.c_uint32), ("power", C.c_uint32), ("norm", C.c_uint32), ("n_chroma", C.c_uint32),
                ("chroma_norm", C.c_uint32), ("reserved", C.c_uint32),
                ("fmin", C.c_double), ("tuning", C.c_double), ("filter_scale", C.c_double), ("gamma", C.c_double)]


VSYN_CQT_SCALE, VSYN_CQT_BASE_C = 1, 2
VSYN_CQT_MAG, VSYN_CQT_COMPLEX, VSYN_CQT_CHROMA, VSYN_CQT_TONNETZ = 1, 2, 3, 4
VSYN_CQT_NOT_FINITE, VSYN_CQT_RATE = 1, 2
VSYN_CQT_RATE_REFUSED = 100  # vsyn_cqt_lengths / vsyn_cqt_basis: step 10 refuses the rate
VSYN_CQT_MAX_LENGTH, VSYN_CQT_MAX_TABLE = 1 << 17, 1 << 23


class TuningSpec(C.Structure):  # vsyn_tuning_spec, 40 bytes
    _fields_ = [("fmin", C.c_double), ("fmax", C.c_double), ("threshold", C.c_double), ("resolution", C.c_double),
                ("bins_per_octave", C.c_uint32), ("reserved", C.c_uint32)]


VSYN_TUNING_ONLY, VSYN_TUNING_ROWS = 0, 1


class LoudnessSpec(C.Structure):  # vsyn_loudness_spec
    _fields_ = [("options", C.c_uint32), ("channel_mode", C.c_uint32), ("target", C.c_double)]


# vsyn_loudness_record
LOUDNESS_RECORD_DTYPE = np.dtype([("zbar", "<f8"), ("zbar_a", "<f8"), ("blocks", "<u4"), ("blocks_abs", "<u4"), ("blocks_rel", "<u4"),
                                  ("gain", "<f4"), ("status", "<u4"), ("reserved", "<u4")])
VSYN_LOUD_NORMALIZE = 1
VSYN_LOUD_SUM, VSYN_LOUD_MONO = 0, 1
VSYN_LOUD_OK, VSYN_LOUD_NOT_FINITE, VSYN_LOUD_TOO_SHORT, VSYN_LOUD_SILENT, VSYN_LOUD_RATE_REFUSED = 0, 1, 2, 3, 4


class Status(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("first_bad_packet", C.c_uint32)]


class Codebook(C.Structure):
    _fields_ = [("dimensions", C.c_uint32), ("num_entries", C.c_uint32), ("lookup", C.POINTER(C.c_float))]


class Residue(C.Structure):
    _fields_ = [("type", C.c_uint32), ("begin", C.c_uint32), ("end", C.c_uint32), ("partition_size", C.c_uint32),
                ("num_classifications", C.c_uint32), ("classwords", C.c_uint32), ("books", C.POINTER(C.c_int16))]


class VqMapping(C.Structure):
    _fields_ = [("num_submaps", C.c_uint32), ("mux", C.POINTER(C.c_uint8)), ("submap_residue", C.POINTER(C.c_uint8))]


class VqSetup(C.Structure):
    _fields_ = [("num_codebooks", C.c_uint32), ("codebooks", C.POINTER(Codebook)),
                ("num_residues", C.c_uint32), ("residues", C.POINTER(Residue)),
                ("num_mappings", C.c_uint32), ("mappings", C.POINTER(VqMapping))]


class VqBatch(C.Structure):
    _fields_ = [("packets", C.c_void_p), ("cls", C.c_void_p), ("entries", C.c_void_p),
                ("num_cls", C.c_uint64), ("num_entries", C.c_uint64)]


class VqSpec:
    """Plain-python description of the residue VQ setup; `.c_setup()` builds the vsyn_vq_setup tree (keeps it alive).
    codebooks: list of (dimensions, num_entries, float32 table [entries*dims] or None)
    residues:  list of dict(type, begin, end, partition_size, num_classifications, classwords, books int16 [nclass*8])
    mappings:  list of (mux list [channels], submap_residue list)"""

    def __init__(self, codebooks, residues, mappings):
        self.codebooks, self.residues, self.mappings = codebooks, residues, mappings
        self._keep = []

    def c_setup(self):
        keep = []
        cb = (Codebook * len(self.codebooks))()
        for i, (dims, n, tab) in enumerate(self.codebooks):
            cb[i].dimensions, cb[i].num_entries = dims, n
            if tab is not None:
                t = np.ascontiguousarray(tab, np.float32)
                keep.append(t)
                cb[i].lookup = t.ctypes.data_as(C.POINTER(C.c_float))
        rs = (Residue * len(self.residues))()
        for i, r in enumerate(self.residues):
            b = np.ascontiguousarray(r["books"], np.int16)
            keep.append(b)
            rs[i].type, rs[i].begin, rs[i].end, rs[i].partition_size = r["type"], r["begin"], r["end"], r["partition_size"]
            rs[i].num_classifications, rs[i].classwords = r["num_classifications"], r["classwords"]
            rs[i].books = b.ctypes.data_as(C.POINTER(C.c_int16))
        mp = (VqMapping * len(self.mappings))()
        for i, (mux, sres) in enumerate(self.mappings):
            m = (C.c_uint8 * len(mux))(*mux)
            sr = (C.c_uint8 * len(sres))(*sres)
            keep += [m, sr]
            mp[i].num_submaps, mp[i].mux, mp[i].submap_residue = len(sres), m, sr
        keep += [cb, rs, mp]
        self._keep.append(keep)
        return VqSetup(len(self.codebooks), cb, len(self.residues), rs, len(self.mappings), mp)


VQ_PACKET_DTYPE = np.dtype([("entry_off", "<u8"), ("num_entries", "<u4"), ("cls_off", "<u4")], align=True)
assert VQ_PACKET_DTYPE.itemsize == 16

# numpy record layouts of the batch PODs (sizes asserted against the header's comments)
PACKET_DTYPE = np.dtype([("mode", "u1"), ("prev_long", "u1"), ("next_long", "u1"), ("reserved0", "u1"),
                         ("floor_used", "<u4"), ("granule", "<i8")], align=True)
SEGMENT_DTYPE = np.dtype([("stream", "<u4"), ("first_packet", "<u4"), ("num_packets", "<u4"), ("flags", "<u4"),
                          ("residue_off", "<u8")], align=True)
assert PACKET_DTYPE.itemsize == 16 and SEGMENT_DTYPE.itemsize == 24


class SetupSpec:
    """Plain-python description of a stream setup; `.c_setup()` builds the vsyn_setup tree (keeps it alive)."""

    def __init__(self, channels, blocksize0, blocksize1, floors, mappings, modes):
        # floors: list of (multiplier, xs list); mappings: list of (couplings [(mag,ang)], channel_floor list)
        # modes: list of (block_flag, mapping)
        self.channels, self.blocksize0, self.blocksize1 = channels, blocksize0, blocksize1
        self.floors, self.mappings, self.modes = floors, mappings, modes
        self._keep = []

    def c_setup(self):
        keep = []
        fl = (Floor1 * len(self.floors))()
        for i, (mult, xs) in enumerate(self.floors):
            arr = (C.c_uint32 * len(xs))(*xs)
            keep.append(arr)
            fl[i].multiplier, fl[i].num_posts, fl[i].xs = mult, len(xs), arr
        mp = (Mapping * len(self.mappings))()
        for i, (coups, chfloor) in enumerate(self.mappings):
            ca = (Coupling * max(1, len(coups)))()
            for k, (m, a) in enumerate(coups):
                ca[k].magnitude, ca[k].angle = m, a
            cf = (C.c_uint8 * self.channels)(*chfloor)
            keep += [ca, cf]
            mp[i].num_couplings, mp[i].couplings, mp[i].channel_floor = len(coups), ca, cf
        md = (Mode * len(self.modes))()
        for i, (bf, m) in enumerate(self.modes):
            md[i].block_flag, md[i].mapping = bf, m
        su = Setup(self.channels, self.blocksize0, self.blocksize1, len(self.floors), fl, len(self.mappings), mp,
                   len(self.modes), md)
        keep += [fl, mp, md]
        self._keep.append(keep)
        return su

    @property
    def ys_stride(self):
        return (max(len(xs) for _, xs in self.floors) + 3) & ~3

    def blocksize_of_mode(self, mode):
        return self.blocksize1 if self.modes[mode][0] else self.blocksize0


_SYMBOLS = [
    "vsyn_version", "vsyn_abi_version", "vsyn_create", "vsyn_destroy", "vsyn_ys_stride", "vsyn_channels", "vsyn_fused_paths",
    "vsyn_const_block_bytes", "vsyn_submit_device", "vsyn_submit_host", "vsyn_sync_status", "vsyn_reset_streams",
    "vsyn_profile_enable", "vsyn_profile_read", "vsyn_imdct_device", "vsyn_host_alloc", "vsyn_host_free",
    "vsyn_attach_vq", "vsyn_submit_device_vq", "vsyn_submit_host_vq", "vsyn_pcm_interleave_device", "vsyn_pcm_abs_sum_host", "vsyn_pcm_fetch_host",
    "vsyn_feature_rows_device", "vsyn_features_device", "vsyn_features_host",
    "vsyn_spectral_num_frames", "vsyn_spectral_device", "vsyn_pcm_spectral_host", "vsyn_spectral_dim", "vsyn_spectral_lin_tile",
    "vsyn_resample_num_frames", "vsyn_resample_device", "vsyn_pcm_resample_host", "vsyn_pcm_resample_spectral_host",
    "vsyn_spectral_post_dim", "vsyn_spectral_post_device", "vsyn_pcm_spectral_post_host",
    "vsyn_pcm_condition_device", "vsyn_pcm_condition_host", "vsyn_pcm_cond_spectral_host",
    "vsyn_pcm_trim_num_frames", "vsyn_pcm_trim_device", "vsyn_pcm_trim_host", "vsyn_pcm_trim_spectral_host",
    "vsyn_pcm_split_max_intervals", "vsyn_pcm_split_device", "vsyn_pcm_split_host", "vsyn_pcm_split_intervals_host",
    "vsyn_pcm_split_spectral_host",
    "vsyn_spectral_pcen_b", "vsyn_spectral_pcen_device", "vsyn_pcm_trim_spectral_pcen_host", "vsyn_pcm_split_spectral_pcen_host",
    "vsyn_pitch_num_frames", "vsyn_pitch_device", "vsyn_pcm_pitch_host",
    "vsyn_pyin_num_frames", "vsyn_pyin_num_bins", "vsyn_pyin_transition", "vsyn_pyin_device", "vsyn_pyin_decode_device", "vsyn_pcm_pyin_host",
    "vsyn_fdesc_num_frames", "vsyn_fdesc_device", "vsyn_pcm_fdesc_host",
    "vsyn_cqt_dim", "vsyn_cqt_num_frames", "vsyn_cqt_lengths", "vsyn_cqt_basis", "vsyn_cq_to_chroma", "vsyn_cqt_tile", "vsyn_cqt_device",
    "vsyn_pcm_cqt_host",
    "vsyn_loudness_num_blocks", "vsyn_loudness_coefficients", "vsyn_loudness_powers", "vsyn_loudness_device", "vsyn_pcm_loudness_host",
    "vsyn_pcm_chain_host", "vsyn_pcm_chain_spectral_host",
    "vsyn_spectral_chroma_dim", "vsyn_chroma_filterbank", "vsyn_spectral_chroma_tile", "vsyn_spectral_chroma_device",
    "vsyn_pcm_chain_chroma_host",
    "vsyn_tuning_check", "vsyn_piptrack_bins", "vsyn_pitch_tuning", "vsyn_piptrack_tile", "vsyn_piptrack_device", "vsyn_tuning_device",
    "vsyn_pcm_tuning_host", "vsyn_pcm_chain_chroma_est_host", "vsyn_pcm_cqt_est_host",
    "vsyn_spectral_hpss_device", "vsyn_pcm_chain_hpss_host",
    "vsyn_onset_peak_windows", "vsyn_tempogram_win_length", "vsyn_tempogram_tile", "vsyn_tempo_from_mean",
    "vsyn_onset_strength_device", "vsyn_onset_peaks_device", "vsyn_tempogram_device", "vsyn_pcm_chain_rhythm_host",
    "vsyn_beat_period", "vsyn_beat_track_device", "vsyn_pcm_chain_beats_host",
    "vsyn_istft_num_samples", "vsyn_istft_device", "vsyn_pcm_hpss_device", "vsyn_pcm_chain_effects_host",
    "vsyn_pv_num_rows", "vsyn_phase_vocoder_device", "vsyn_stretch_num_samples", "vsyn_pcm_stretch_device", "vsyn_pcm_chain_stretch_host",
]


def _spec_dim(spec, chroma=None):
    from .spectral import CHROMA_KINDS, chroma_spec, spec_dim  # the one formula (spectral imports this module lazily as well)
    if chroma is None and spec.kind in CHROMA_KINDS.values():
        chroma = chroma_spec()  # an entry without the chroma argument serves these kinds with the defaults
    return spec_dim(spec, chroma)


def declared_symbols():
    return list(_SYMBOLS)


_lib = None


def load():
    """dlopen the HIP library. Raises (never falls back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # PyTorch-ROCm bundles its own libamdhip64: when torch shares the process it must be the HIP runtime that
        # gets loaded (two runtimes in one process cannot both own the GPU). Plumbing only; torch is optional.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("HIP extension missing: %s — run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, u32, u64, cpp = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_char_p)
    lib.vsyn_version.restype = C.c_char_p
    lib.vsyn_abi_version.restype = C.c_int
    lib.vsyn_create.argtypes = [C.POINTER(Setup), C.c_int, u32, C.POINTER(vp), cpp]
    lib.vsyn_destroy.argtypes = [vp]
    lib.vsyn_destroy.restype = None
    lib.vsyn_ys_stride.argtypes = [vp]
    lib.vsyn_ys_stride.restype = u32
    lib.vsyn_channels.argtypes = [vp]
    lib.vsyn_channels.restype = u32
    lib.vsyn_const_block_bytes.argtypes = [vp]
    lib.vsyn_const_block_bytes.restype = C.c_size_t
    lib.vsyn_fused_paths.argtypes = [vp]
    lib.vsyn_fused_paths.restype = u32
    lib.vsyn_submit_device.argtypes = [vp, u32, vp, u32, vp, u32, vp, vp, vp, u64, vp, C.POINTER(Taps), u32, vp, cpp]
    lib.vsyn_submit_host.argtypes = [vp, u32, vp, u32, vp, vp, vp, C.c_size_t, vp, u64, vp, C.POINTER(Taps), u32,
                                     C.POINTER(Status), cpp]
    lib.vsyn_sync_status.argtypes = [vp, vp, C.POINTER(Status), cpp]
    lib.vsyn_reset_streams.argtypes = [vp, vp, cpp]
    lib.vsyn_profile_enable.argtypes = [vp, C.c_int]
    lib.vsyn_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u32), cpp]
    lib.vsyn_imdct_device.argtypes = [vp, u32, u32, vp, vp, vp, cpp]
    lib.vsyn_attach_vq.argtypes = [vp, C.POINTER(VqSetup), cpp]
    lib.vsyn_submit_device_vq.argtypes = [vp, u32, vp, u32, vp, u32, vp, C.POINTER(VqBatch), vp, vp, u64, vp,
                                          C.POINTER(Taps), u32, vp, cpp]
    lib.vsyn_submit_host_vq.argtypes = [vp, u32, vp, u32, vp, vp, C.POINTER(VqBatch), vp, C.c_size_t, vp, u64, vp,
                                        C.POINTER(Taps), u32, C.POINTER(Status), cpp]
    lib.vsyn_pcm_interleave_device.argtypes = [vp, C.c_int, vp, u64, vp, u64, vp, vp, cpp]
    lib.vsyn_pcm_abs_sum_host.argtypes = [vp, C.POINTER(C.c_double), cpp]
    lib.vsyn_pcm_fetch_host.argtypes = [vp, C.c_int, vp, u64, vp, cpp]
    lib.vsyn_feature_rows_device.argtypes = [vp, C.POINTER(FeatureSpec), u32, vp, u32, vp, u32, vp, vp, cpp]
    lib.vsyn_features_device.argtypes = [vp, C.POINTER(FeatureSpec), u32, vp, u32, vp, u32, vp, vp, vp, vp, vp, cpp]
    lib.vsyn_features_host.argtypes = [vp, C.POINTER(FeatureSpec), u32, vp, u32, vp, vp, vp, C.c_size_t, vp, u64, vp,
                                       C.POINTER(Status), cpp]
    lib.vsyn_spectral_num_frames.argtypes = [C.POINTER(SpectralSpec), u64]
    lib.vsyn_spectral_num_frames.restype = u64
    lib.vsyn_spectral_dim.argtypes = [C.POINTER(SpectralSpec)]
    lib.vsyn_spectral_dim.restype = u32
    lib.vsyn_spectral_lin_tile.argtypes = [C.POINTER(SpectralSpec)]
    lib.vsyn_spectral_lin_tile.restype = u32
    lib.vsyn_spectral_device.argtypes = [vp, C.POINTER(SpectralSpec), u32, vp, vp, u64, u32, vp, vp, vp, vp, cpp]
    lib.vsyn_pcm_spectral_host.argtypes = [vp, C.POINTER(SpectralSpec), u32, vp, vp, u64, vp, C.POINTER(Status), cpp]
    lib.vsyn_resample_num_frames.argtypes = [u32, u32, u64]
    lib.vsyn_resample_num_frames.restype = u64
    lib.vsyn_resample_device.argtypes = [vp, u32, vp, u32, vp, u64, u32, vp, vp, u64, vp, vp, cpp]
    lib.vsyn_pcm_resample_host.argtypes = [vp, u32, vp, u32, C.c_int, vp, u64, vp, cpp]
    lib.vsyn_pcm_resample_spectral_host.argtypes = [vp, C.POINTER(SpectralSpec), u32, vp, u32, vp, u64, vp, C.POINTER(Status), cpp]
    lib.vsyn_spectral_post_dim.argtypes = [C.POINTER(SpectralSpec), C.POINTER(SpectralPost)]
    lib.vsyn_spectral_post_dim.restype = u32
    lib.vsyn_spectral_post_device.argtypes = [vp, C.POINTER(SpectralPost), u32, u32, vp, vp, vp, vp, cpp]
    lib.vsyn_pcm_spectral_post_host.argtypes = [vp, C.POINTER(SpectralSpec), C.POINTER(SpectralPost), u32, vp, u32, vp, u64, vp,
                                                C.POINTER(Status), cpp]
    lib.vsyn_pcm_condition_device.argtypes = [vp, C.POINTER(PcmCond), u32, vp, u64, u32, vp, vp, u64, vp, vp, cpp]
    lib.vsyn_pcm_condition_host.argtypes = [vp, C.POINTER(PcmCond), u32, vp, u32, C.c_int, vp, u64, vp, vp, cpp]
    lib.vsyn_pcm_cond_spectral_host.argtypes = [vp, C.POINTER(PcmCond), C.POINTER(SpectralSpec), C.POINTER(SpectralPost), u32, vp, u32, vp,
                                                u64, vp, vp, C.POINTER(Status), cpp]
    lib.vsyn_pcm_trim_num_frames.argtypes = [C.POINTER(PcmTrim), u64]
    lib.vsyn_pcm_trim_num_frames.restype = u64
    lib.vsyn_pcm_trim_device.argtypes = [vp, C.POINTER(PcmTrim), u32, vp, u64, u32, vp, vp, u64, vp, vp, vp, vp, u64, vp, cpp]
    lib.vsyn_pcm_trim_host.argtypes = [vp, C.POINTER(PcmTrim), C.POINTER(PcmCond), u32, vp, u32, C.c_int, vp, u64, vp, vp, vp, vp, cpp]
    lib.vsyn_pcm_trim_spectral_host.argtypes = [vp, C.POINTER(PcmTrim), C.POINTER(PcmCond), C.POINTER(SpectralSpec), C.POINTER(SpectralPost),
                                                u32, vp, u32, vp, u64, vp, vp, vp, vp, C.POINTER(Status), cpp]
    lib.vsyn_pcm_split_max_intervals.argtypes = [C.POINTER(PcmTrim), u64]
    lib.vsyn_pcm_split_max_intervals.restype = u64
    lib.vsyn_pcm_split_device.argtypes = [vp, C.POINTER(PcmTrim), u32, vp, u64, u32, vp, vp, u64, vp, vp, vp, u64, vp, vp, u64, vp, cpp]
    lib.vsyn_pcm_split_host.argtypes = [vp, C.POINTER(PcmTrim), C.POINTER(PcmCond), u32, vp, u32, C.c_int, vp, u64, vp, vp, vp, u64, vp, vp, cpp]
    lib.vsyn_pcm_split_intervals_host.argtypes = [vp, C.POINTER(PcmTrim), u32, vp, u32, vp, vp, vp, u64, vp, cpp]
    lib.vsyn_pcm_split_spectral_host.argtypes = [vp, C.POINTER(PcmTrim), C.POINTER(PcmCond), C.POINTER(SpectralSpec), C.POINTER(SpectralPost),
                                                 u32, vp, u32, vp, u64, vp, vp, vp, vp, u64, vp, vp, C.POINTER(Status), cpp]
    lib.vsyn_spectral_pcen_b.argtypes = [C.POINTER(SpectralPcen), u32, u32]
    lib.vsyn_spectral_pcen_b.restype = C.c_double
    lib.vsyn_spectral_pcen_device.argtypes = [vp, C.POINTER(SpectralPcen), u32, u32, vp, vp, u32, vp, vp, vp, cpp]
    lib.vsyn_pcm_trim_spectral_pcen_host.argtypes = [vp, C.POINTER(PcmTrim), C.POINTER(PcmCond), C.POINTER(SpectralSpec), C.POINTER(SpectralPcen),
                                                     C.POINTER(SpectralPost), u32, vp, u32, vp, u64, vp, vp, vp, vp, C.POINTER(Status), cpp]
    lib.vsyn_pcm_split_spectral_pcen_host.argtypes = [vp, C.POINTER(PcmTrim), C.POINTER(PcmCond), C.POINTER(SpectralSpec), C.POINTER(SpectralPcen),
                                                      C.POINTER(SpectralPost), u32, vp, u32, vp, u64, vp, vp, vp, vp, u64, vp, vp,
                                                      C.POINTER(Status), cpp]
    lib.vsyn_pitch_num_frames.argtypes = [C.POINTER(PitchSpec), u64]
    lib.vsyn_pitch_num_frames.restype = u64
    lib.vsyn_pitch_device.argtypes = [vp, C.POINTER(PitchSpec), u32, vp, vp, u64, u32, vp, vp, vp, vp, vp, cpp]
    lib.vsyn_pcm_pitch_host.argtypes = [vp, C.POINTER(PitchSpec), u32, vp, u32, vp, u64, vp, vp, C.POINTER(Status), cpp]
    lib.vsyn_pyin_num_frames.argtypes = [C.POINTER(PyinSpec), u64]
    lib.vsyn_pyin_num_frames.restype = u64
    lib.vsyn_pyin_num_bins.argtypes = [C.POINTER(PyinSpec)]
    lib.vsyn_pyin_num_bins.restype = u32
    lib.vsyn_pyin_transition.argtypes = [C.POINTER(PyinSpec), u32, vp, vp, vp, u64, cpp]
    lib.vsyn_pyin_device.argtypes = [vp, C.POINTER(PyinSpec), u32, vp, vp, u64, u32, vp, vp, vp, vp, vp, cpp]
    lib.vsyn_pyin_decode_device.argtypes = [vp, C.POINTER(PyinSpec), u32, vp, vp, vp, vp, vp, cpp]
    lib.vsyn_pcm_pyin_host.argtypes = [vp, C.POINTER(PyinSpec), u32, vp, u32, vp, u64, vp, vp, C.POINTER(Status), cpp]
    lib.vsyn_fdesc_num_frames.argtypes = [C.POINTER(FdescSpec), u64]
    lib.vsyn_fdesc_num_frames.restype = u64
    lib.vsyn_fdesc_device.argtypes = [vp, C.POINTER(FdescSpec), u32, vp, vp, u64, u32, vp, vp, vp, vp, vp, cpp]
    lib.vsyn_pcm_fdesc_host.argtypes = [vp, C.POINTER(FdescSpec), u32, vp, u32, vp, u64, vp, vp, C.POINTER(Status), cpp]
    lib.vsyn_cqt_dim.argtypes = [C.POINTER(CqtSpec)]
    lib.vsyn_cqt_dim.restype = u32
    lib.vsyn_cqt_num_frames.argtypes = [C.POINTER(CqtSpec), u64]
    lib.vsyn_cqt_num_frames.restype = u64
    lib.vsyn_cqt_lengths.argtypes = [u32, C.POINTER(CqtSpec), vp, vp]
    lib.vsyn_cqt_basis.argtypes = [u32, C.POINTER(CqtSpec), u32, vp]
    lib.vsyn_cq_to_chroma.argtypes = [C.POINTER(CqtSpec), vp]
    lib.vsyn_cqt_tile.argtypes = [C.POINTER(CqtSpec), u32, vp]
    lib.vsyn_cqt_device.argtypes = [vp, C.POINTER(CqtSpec), u32, vp, vp, u64, u32, vp, vp, vp, vp, vp, cpp]
    lib.vsyn_pcm_cqt_host.argtypes = [vp, C.POINTER(CqtSpec), u32, vp, u32, vp, u64, vp, vp, C.POINTER(Status), cpp]
    lib.vsyn_pcm_cqt_est_host.argtypes = [vp, C.POINTER(CqtSpec), C.POINTER(TuningSpec), u32, vp, u32, vp, u64, vp, vp, vp, C.POINTER(Status), cpp]
    lib.vsyn_loudness_num_blocks.argtypes = [u32, u64]
    lib.vsyn_loudness_num_blocks.restype = u64
    lib.vsyn_loudness_coefficients.argtypes = [u32, vp]
    lib.vsyn_loudness_powers.argtypes = [u32, vp]
    lib.vsyn_loudness_device.argtypes = [vp, C.POINTER(LoudnessSpec), u32, vp, vp, vp, u64, u32, vp, vp, vp, u64, vp, u64, vp, cpp]
    lib.vsyn_pcm_loudness_host.argtypes = [vp, C.POINTER(LoudnessSpec), u32, vp, u32, vp, vp, u64, vp, C.POINTER(Status), cpp]
    lib.vsyn_pcm_chain_host.argtypes = [vp, C.POINTER(PcmTrim), C.c_int, C.POINTER(LoudnessSpec), C.POINTER(PcmCond), u32, vp, u32, C.c_int, vp,
                                        u64, vp, vp, vp, vp, u64, vp, vp, vp, cpp]
    lib.vsyn_pcm_chain_spectral_host.argtypes = [vp, C.POINTER(PcmTrim), C.c_int, C.POINTER(LoudnessSpec), C.POINTER(PcmCond),
                                                 C.POINTER(SpectralSpec), C.POINTER(SpectralPcen), C.POINTER(SpectralPost), u32, vp, u32, vp, u64,
                                                 vp, vp, vp, vp, vp, u64, vp, vp, vp, C.POINTER(Status), cpp]
    lib.vsyn_spectral_chroma_dim.argtypes = [C.POINTER(SpectralSpec), C.POINTER(SpectralChroma)]
    lib.vsyn_spectral_chroma_dim.restype = u32
    lib.vsyn_chroma_filterbank.argtypes = [u32, C.POINTER(SpectralSpec), C.POINTER(SpectralChroma), vp]
    lib.vsyn_spectral_chroma_tile.argtypes = [C.POINTER(SpectralSpec)]
    lib.vsyn_spectral_chroma_tile.restype = u32
    lib.vsyn_spectral_chroma_device.argtypes = [vp, C.POINTER(SpectralSpec), C.POINTER(SpectralChroma), u32, vp, vp, u64, u32, vp, vp, vp, vp, cpp]
    lib.vsyn_pcm_chain_chroma_host.argtypes = [vp, C.POINTER(PcmTrim), C.c_int, C.POINTER(LoudnessSpec), C.POINTER(PcmCond),
                                               C.POINTER(SpectralSpec), C.POINTER(SpectralChroma), C.POINTER(SpectralPcen),
                                               C.POINTER(SpectralPost), u32, vp, u32, vp, u64, vp, vp, vp, vp, vp, u64, vp, vp, vp,
                                               C.POINTER(Status), cpp]
    lib.vsyn_tuning_check.argtypes = [C.POINTER(SpectralSpec), C.POINTER(TuningSpec), cpp]
    lib.vsyn_piptrack_bins.argtypes = [u32, C.POINTER(SpectralSpec), C.POINTER(TuningSpec), vp]
    lib.vsyn_pitch_tuning.argtypes = [vp, vp, u64, C.c_double, u32, vp, vp]
    lib.vsyn_piptrack_tile.argtypes = [C.POINTER(SpectralSpec)]
    lib.vsyn_piptrack_tile.restype = u32
    lib.vsyn_piptrack_device.argtypes = [vp, C.POINTER(SpectralSpec), C.POINTER(TuningSpec), u32, vp, vp, u64, u32, vp, vp, vp, vp, vp, cpp]
    lib.vsyn_tuning_device.argtypes = [vp, C.POINTER(SpectralSpec), C.POINTER(TuningSpec), u32, vp, vp, u64, u32, vp, vp, vp, vp, cpp]
    lib.vsyn_pcm_tuning_host.argtypes = [vp, C.POINTER(SpectralSpec), C.POINTER(TuningSpec), u32, vp, u32, u32, vp, vp, vp, u64, vp,
                                         C.POINTER(Status), cpp]
    lib.vsyn_pcm_chain_chroma_est_host.argtypes = [vp, C.POINTER(PcmTrim), C.c_int, C.POINTER(LoudnessSpec), C.POINTER(PcmCond),
                                                   C.POINTER(SpectralSpec), C.POINTER(SpectralChroma), C.POINTER(SpectralPcen),
                                                   C.POINTER(SpectralPost), C.POINTER(TuningSpec), u32, vp, u32, vp, u64, vp, vp, vp, vp, vp,
                                                   u64, vp, vp, vp, vp, C.POINTER(Status), cpp]
    lib.vsyn_spectral_hpss_device.argtypes = [vp, C.POINTER(SpectralHpss), u32, u32, vp, vp, vp, vp, cpp]
    lib.vsyn_istft_num_samples.argtypes = [C.POINTER(SpectralSpec), u64]
    lib.vsyn_istft_num_samples.restype = u64
    lib.vsyn_istft_device.argtypes = [vp, C.POINTER(SpectralSpec), u32, vp, vp, vp, vp, vp, u64, vp, vp, cpp]
    lib.vsyn_pcm_hpss_device.argtypes = [vp, C.POINTER(PcmEffect), u32, vp, vp, u64, u32, vp, u64, vp, vp, cpp]
    lib.vsyn_pcm_chain_effects_host.argtypes = [vp, C.POINTER(PcmTrim), C.c_int, C.POINTER(PcmEffect), C.POINTER(LoudnessSpec), C.POINTER(PcmCond), u32,
                                                vp, u32, C.c_int, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp, cpp]
    lib.vsyn_pv_num_rows.argtypes = [u64, C.c_double]
    lib.vsyn_pv_num_rows.restype = u64
    lib.vsyn_phase_vocoder_device.argtypes = [vp, C.POINTER(SpectralSpec), u32, vp, vp, vp, vp, vp, vp, cpp]
    lib.vsyn_stretch_num_samples.argtypes = [u64, C.c_double]
    lib.vsyn_stretch_num_samples.restype = u64
    lib.vsyn_pcm_stretch_device.argtypes = [vp, C.POINTER(PcmStretch), u32, vp, vp, vp, vp, u64, u32, vp, u64, vp, vp, cpp]
    lib.vsyn_pcm_chain_stretch_host.argtypes = [vp, C.POINTER(PcmTrim), C.c_int, C.POINTER(PcmEffect), C.POINTER(PcmStretch), vp, vp,
                                                C.POINTER(LoudnessSpec), C.POINTER(PcmCond), u32, vp, u32, C.c_int, vp, u64, vp, vp, vp, vp, u64, vp,
                                                vp, vp, cpp]
    lib.vsyn_pcm_chain_hpss_host.argtypes = [vp, C.POINTER(PcmTrim), C.c_int, C.POINTER(LoudnessSpec), C.POINTER(PcmCond),
                                             C.POINTER(SpectralSpec), C.POINTER(SpectralChroma), C.POINTER(SpectralHpss),
                                             C.POINTER(SpectralPcen), C.POINTER(SpectralPost), u32, vp, u32, vp, u64, vp, vp, vp, vp, vp, u64,
                                             vp, vp, vp, C.POINTER(Status), cpp]
    lib.vsyn_onset_peak_windows.argtypes = [C.POINTER(OnsetPeaks), u32, vp, cpp]
    lib.vsyn_tempogram_win_length.argtypes = [C.POINTER(TempogramSpec), u32]
    lib.vsyn_tempogram_win_length.restype = u32
    lib.vsyn_tempogram_tile.argtypes = [u32]
    lib.vsyn_tempogram_tile.restype = u32
    lib.vsyn_tempo_from_mean.argtypes = [C.POINTER(TempoSpec), vp, u32, u32, u32, C.POINTER(C.c_double), C.POINTER(u32), cpp]
    lib.vsyn_onset_strength_device.argtypes = [vp, C.POINTER(OnsetSpec), u32, u32, vp, vp, vp, vp, cpp]
    lib.vsyn_onset_peaks_device.argtypes = [vp, C.POINTER(OnsetPeaks), u32, vp, vp, vp, vp, vp, vp, vp, cpp]
    lib.vsyn_tempogram_device.argtypes = [vp, C.POINTER(TempogramSpec), u32, vp, vp, vp, vp, vp, vp, cpp]
    lib.vsyn_pcm_chain_rhythm_host.argtypes = [vp, C.POINTER(PcmTrim), C.c_int, C.POINTER(LoudnessSpec), C.POINTER(PcmCond),
                                               C.POINTER(SpectralSpec), C.POINTER(SpectralChroma), C.POINTER(SpectralHpss),
                                               C.POINTER(SpectralPcen), C.POINTER(SpectralPost), C.POINTER(RhythmSpec), u32, vp, u32, vp, u64, vp,
                                               vp, vp, vp, vp, u64, vp, vp, vp, vp, C.POINTER(Status), cpp]
    lib.vsyn_beat_period.argtypes = [C.POINTER(BeatSpec), C.c_double, u32, C.POINTER(u32), cpp]
    lib.vsyn_beat_track_device.argtypes = [vp, C.POINTER(BeatSpec), u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, cpp]
    lib.vsyn_pcm_chain_beats_host.argtypes = [vp, C.POINTER(PcmTrim), C.c_int, C.POINTER(LoudnessSpec), C.POINTER(PcmCond),
                                              C.POINTER(SpectralSpec), C.POINTER(SpectralChroma), C.POINTER(SpectralHpss),
                                              C.POINTER(SpectralPcen), C.POINTER(SpectralPost), C.POINTER(OnsetSpec), C.POINTER(BeatSpec), u32, vp,
                                              u32, vp, u64, vp, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, C.POINTER(Status), cpp]
    lib.vsyn_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp), cpp]
    lib.vsyn_host_free.argtypes = [vp]
    lib.vsyn_host_free.restype = None
    _lib = lib
    return lib


def onset_peak_windows(peaks, sample_rate):
    """vsyn_onset_peak_windows: (pre_max, post_max, pre_avg, post_avg, wait) in frames for one rate. Host arithmetic, no GPU."""
    out, err = np.zeros(5, np.uint32), C.c_char_p()
    _check(load().vsyn_onset_peak_windows(C.byref(peaks), sample_rate, _ptr(out), C.byref(err)), err)
    return tuple(int(v) for v in out)


def tempo_from_mean(tempo, g, sample_rate, hop_length):
    """vsyn_tempo_from_mean of one mean tempogram g (float64, W values): (bpm, lag). Host arithmetic, no GPU."""
    g = np.ascontiguousarray(g, dtype=np.float64)
    bpm, lag, err = C.c_double(), C.c_uint32(), C.c_char_p()
    _check(load().vsyn_tempo_from_mean(C.byref(tempo), _ptr(g), len(g), sample_rate, hop_length, C.byref(bpm), C.byref(lag), C.byref(err)), err)
    return bpm.value, lag.value


def beat_period(beat, bpm, sample_rate):
    """vsyn_beat_period: the beat period in frames for one tempo and rate, 0 for one outside [1, 2048]. Host arithmetic, no GPU."""
    P, err = C.c_uint32(), C.c_char_p()
    _check(load().vsyn_beat_period(C.byref(beat), float(bpm), int(sample_rate), C.byref(P), C.byref(err)), err)
    return P.value


class VsynError(RuntimeError):
    def __init__(self, code, msg, status=None):
        super().__init__("vsyn error %d: %s" % (code, msg))
        self.code, self.status = code, status


def _check(rc, err, ok=(VSYN_OK,)):
    if rc not in ok:
        raise VsynError(rc, (err.value or b"").decode())


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _ref(x):
    return None if x is None else C.byref(x)


def _rates(r):
    return None if r is None else np.ascontiguousarray(r, dtype=np.uint32)


def cqt_lengths(spec, sample_rate):
    """vsyn_cqt_lengths (host only, no device): (rc, N float64 [n_bins], L uint32 [n_bins]); rc is VSYN_OK, VSYN_CQT_RATE_REFUSED
    (step 10) or VSYN_ERR_INVALID (the spec, a rate of 0: N and L zeros; or a cap of step 11: N and L filled)."""
    n = max(1, min(int(spec.n_bins), 256))
    N, L = np.zeros(n, np.float64), np.zeros(n, np.uint32)
    rc = load().vsyn_cqt_lengths(sample_rate, C.byref(spec), _ptr(N), _ptr(L))
    return rc, N, L


def cqt_basis(spec, sample_rate, k):
    """vsyn_cqt_basis (host only): bin k's wavelet as complex64 [L_k], what the device's table holds. Raises VsynError unless VSYN_OK."""
    rc, _, L = cqt_lengths(spec, sample_rate)
    if rc != VSYN_OK or not 0 <= k < spec.n_bins:
        raise VsynError(rc or VSYN_ERR_INVALID, "vsyn_cqt_lengths refuses the spec, the rate or the bin")
    out = np.zeros(2 * int(L[k]), np.float32)
    rc = load().vsyn_cqt_basis(sample_rate, C.byref(spec), k, _ptr(out))
    if rc != VSYN_OK:
        raise VsynError(rc, "vsyn_cqt_basis")
    return out.view(np.complex64)


def cq_to_chroma(spec):
    """vsyn_cq_to_chroma (host only): the 0/1 fold matrix float32 (n_chroma, n_bins). Raises VsynError for an invalid spec."""
    if not (1 <= spec.n_bins <= 256 and 1 <= spec.n_chroma <= 256):
        raise VsynError(VSYN_ERR_INVALID, "n_bins or n_chroma outside [1, 256]")
    out = np.zeros((int(spec.n_chroma), int(spec.n_bins)), np.float32)
    rc = load().vsyn_cq_to_chroma(C.byref(spec), _ptr(out))
    if rc != VSYN_OK:
        raise VsynError(rc, "vsyn_cq_to_chroma")
    return out


def tuning_check(spec, tun):
    """vsyn_tuning_check (host only): raises VsynError naming what "tuning estimation" step 9 refuses."""
    err = C.c_char_p()
    _check(load().vsyn_tuning_check(C.byref(spec), C.byref(tun), C.byref(err)), err)


def piptrack_bins(sample_rate, spec, tun):
    """vsyn_piptrack_bins (host only): (k_lo, k_hi) of the searched band at sample_rate."""
    out = np.zeros(2, np.uint32)
    rc = load().vsyn_piptrack_bins(int(sample_rate), C.byref(spec), C.byref(tun), _ptr(out))
    if rc != VSYN_OK:
        raise VsynError(rc, "vsyn_piptrack_bins refuses the rate, the spec or the tuning spec")
    return int(out[0]), int(out[1])


def pitch_tuning(freqs, mags=None, resolution=0.01, bins_per_octave=12):
    """vsyn_pitch_tuning (host only): (tuning, n, selected) of float32 freqs (and mags, or None: every freqs > 0 is selected)."""
    f = np.ascontiguousarray(freqs, np.float32).reshape(-1)
    m = None if mags is None else np.ascontiguousarray(mags, np.float32).reshape(-1)
    if m is not None and m.size != f.size:
        raise ValueError("freqs and mags differ in size")
    t, cnt = np.zeros(1, np.float64), np.zeros(2, np.uint64)
    rc = load().vsyn_pitch_tuning(_ptr(f) if f.size else None, _ptr(m) if m is not None and m.size else None, f.size, float(resolution),
                                  int(bins_per_octave), _ptr(t), _ptr(cnt))
    if rc != VSYN_OK:
        raise VsynError(rc, "vsyn_pitch_tuning refuses resolution %r or bins_per_octave %r" % (resolution, bins_per_octave))
    return float(t[0]), int(cnt[0]), int(cnt[1])


def cqt_tile(spec, sample_rate):
    """vsyn_cqt_tile (host only): (frames per workgroup, samples per chunk, bins per workgroup)."""
    out = np.zeros(3, np.uint32)
    rc = load().vsyn_cqt_tile(C.byref(spec), sample_rate, _ptr(out))
    if rc != VSYN_OK:
        raise VsynError(rc, "vsyn_cqt_tile")
    return int(out[0]), int(out[1]), int(out[2])


_PER_SEGMENT = dict(frames=(np.uint64,), seg_rows=(np.uint64,), peaks=(np.float32,), refs=(np.float64,), counts=(np.uint32,),
                    refused=(np.uint32,), bounds=(np.uint32, 2))


def _per_segment(S, *names):
    """The named per-segment outputs of a host entry, zeroed and never empty (C gets their pointers)."""
    return {n: np.zeros((max(1, S),) + _PER_SEGMENT[n][1:], _PER_SEGMENT[n][0]) for n in names}


def _post_dim(spec, post, chroma=None):
    return _spec_dim(spec, chroma) * (1 + (post.order if post is not None else 0))


class Synth:
    """Owns one vsyn_handle. Thin: every method is one C-ABI call (a host entry that sizes its own output: two, _sized_call)."""

    def __init__(self, spec, device=0, max_streams=64):
        self.lib = load()
        self.spec = spec
        self._su = spec.c_setup()
        h, err = C.c_void_p(), C.c_char_p()
        _check(self.lib.vsyn_create(C.byref(self._su), device, max_streams, C.byref(h), C.byref(err)), err)
        self.h = h
        self.channels = spec.channels
        self.ys_stride = self.lib.vsyn_ys_stride(h)
        self.fused_paths = self.lib.vsyn_fused_paths(h)  # bit 0: fused kernel for long-block runs, bit 1: for mixed-block runs too

    def close(self):
        if getattr(self, "h", None):
            self.lib.vsyn_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self, stream=None):
        err = C.c_char_p()
        _check(self.lib.vsyn_reset_streams(self.h, stream, C.byref(err)), err)

    def submit_host(self, packets, segments, ys, residue, plane_stride, want_taps=False, flags=0):
        """numpy in, numpy out: returns dict(pcm [S][C][plane_stride], emit_len [P], taps..., status)."""
        P, S, Cn = len(packets), len(segments), self.channels
        packets = np.ascontiguousarray(packets, dtype=PACKET_DTYPE)
        segments = np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE)
        ys = np.ascontiguousarray(ys, dtype=np.uint16)
        residue = np.ascontiguousarray(residue, dtype=np.float32)
        assert ys.size == P * Cn * self.ys_stride
        pcm = np.zeros((S, Cn, plane_stride), np.float32)
        emit = np.zeros(P, np.uint32)
        taps, tp = None, None
        if want_taps == "features":  # the two feature taps only (they do not force the staged kernels)
            taps = dict(floor_final=np.zeros(ys.size, np.uint16), floor_curve=np.zeros(residue.size, np.uint16))
            tp = Taps(None, None, taps["floor_final"].ctypes.data, taps["floor_curve"].ctypes.data)
        elif want_taps:
            taps = dict(after_envelope=np.zeros(residue.size, np.float32),
                        pcm_after_mdct=np.zeros(residue.size * 2, np.float32),
                        floor_final=np.zeros(ys.size, np.uint16),
                        floor_curve=np.zeros(residue.size, np.uint16))
            tp = Taps(taps["after_envelope"].ctypes.data, taps["pcm_after_mdct"].ctypes.data,
                      taps["floor_final"].ctypes.data, taps["floor_curve"].ctypes.data)
        st, err = Status(), C.c_char_p()
        rc = self.lib.vsyn_submit_host(self.h, P, _ptr(packets), S, _ptr(segments), _ptr(ys), _ptr(residue),
                                       residue.size, _ptr(pcm), plane_stride, _ptr(emit),
                                       C.byref(tp) if tp else None, flags, C.byref(st), C.byref(err))
        _check(rc, err, (VSYN_OK, VSYN_ERR_STREAM))
        return dict(rc=rc, pcm=pcm, emit_len=emit, taps=taps, flags=st.flags, first_bad=st.first_bad_packet)

    def features_host(self, spec, packets, segments, ys, residue=None):
        """vsyn_features_host with a FeatureSpec: returns dict(rc, rows [total][output_dim], seg_rows [S], flags, first_bad)."""
        P, S, Cn = len(packets), len(segments), self.channels
        packets = np.ascontiguousarray(packets, dtype=PACKET_DTYPE)
        segments = np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE)
        ys = np.ascontiguousarray(ys, dtype=np.uint16)
        assert ys.size == P * Cn * self.ys_stride
        if residue is not None:
            residue = np.ascontiguousarray(residue, dtype=np.float32)
        rows = np.zeros((max(1, P * Cn), spec.output_dim), np.float32)
        seg_rows = np.zeros(max(1, S), np.uint64)
        st, err = Status(), C.c_char_p()
        rc = self.lib.vsyn_features_host(self.h, C.byref(spec), P, _ptr(packets), S, _ptr(segments), _ptr(ys), _ptr(residue),
                                         0 if residue is None else residue.size, _ptr(rows), rows.shape[0], _ptr(seg_rows),
                                         C.byref(st), C.byref(err))
        _check(rc, err, (VSYN_OK, VSYN_ERR_STREAM))
        total = int(seg_rows[:S].sum()) if rc == VSYN_OK else 0
        return dict(rc=rc, rows=rows[:total], seg_rows=seg_rows[:S], flags=st.flags, first_bad=st.first_bad_packet)

    def _sized_call(self, fn, head, sizes, alloc, st=None, ok=(VSYN_OK,)):
        """The two calls of a host entry fn(h, *head, buffer, its capacity or stride, sizes, further outputs ..., [status,] err): with
        a NULL buffer (and every further output NULL or 0) for sizes [S], the frames or the row counts; then (buffer, n, outs) =
        alloc() and the call that fills them. Returns (rc of the second call, buffer)."""
        err = C.c_char_p()
        tail = ([] if st is None else [C.byref(st)]) + [C.byref(err)]
        nulls = [0] * (len(fn.argtypes) - len(head) - len(tail) - 4)
        _check(fn(self.h, *head, None, 0, _ptr(sizes), *nulls, *tail), err)
        buf, n, outs = alloc()
        rc = fn(self.h, *head, _ptr(buf), n, _ptr(sizes), *[_ptr(o) if isinstance(o, np.ndarray) else o for o in outs], *tail)
        _check(rc, err, ok)
        return rc, buf

    def _rows_host(self, fn, head, S, cols, outs=(), named={}):
        """A host entry that returns rows: dict(rc, rows [total][cols], seg_rows [S], flags) and the named per-segment outputs; outs
        are its further outputs in the order of the C arguments."""
        seg_rows, st = np.zeros(max(1, S), np.uint64), Status()
        rc, rows = self._sized_call(fn, head, seg_rows, lambda: (np.zeros((max(1, int(seg_rows[:S].sum())), cols), np.float32),
                                                                 int(seg_rows[:S].sum()), outs), st, (VSYN_OK, VSYN_ERR_STREAM))
        return dict(rc=rc, rows=rows[:int(seg_rows[:S].sum())], seg_rows=seg_rows[:S], flags=st.flags, **{k: v[:S] for k, v in named.items()})

    def _pcm_host(self, fn, head, S, fmt, chans, outs):
        """A host entry that returns PCM: (pcm, frames [S]); pcm is float32 [S][chans][stride] (planar) or int16 [S][stride][chans]
        (interleaved), for chans = None (mono) [S][stride] of either, stride = the largest of the frames the size query gives.
        outs(t_max): its further outputs in the order of the C arguments."""
        frames = np.zeros(max(1, S), np.uint64)

        def alloc():
            t_max = int(frames[:S].max()) if S else 0
            stride = max(1, t_max)
            shape = (S, stride) if chans is None else (S, chans, stride) if fmt == VSYN_PCM_F32 else (S, stride, chans)
            return np.zeros(shape, np.float32 if fmt == VSYN_PCM_F32 else np.int16), stride, outs(t_max)
        return self._sized_call(fn, head, frames, alloc)[1], frames[:S]

    def pcm_spectral_host(self, spec, sample_rates):
        """vsyn_pcm_spectral_host over the last submit's segments: returns dict(rc, rows [total][dim], seg_rows [S], flags)."""
        rates = _rates(sample_rates)
        return self._rows_host(self.lib.vsyn_pcm_spectral_host, (C.byref(spec), len(rates), _ptr(rates)), len(rates), _spec_dim(spec))

    def spectral_device(self, spec, sample_rates, d_pcm, plane_stride, channels, d_frames, d_rows, d_seg_row_off=None, stream=None):
        """vsyn_spectral_device on device pointers (ints); sample_rates is a host sequence."""
        rates = _rates(sample_rates)
        err = C.c_char_p()
        _check(self.lib.vsyn_spectral_device(self.h, C.byref(spec), len(rates), _ptr(rates), d_pcm, plane_stride, channels, d_frames, d_rows,
                                             d_seg_row_off, stream, C.byref(err)), err)

    def spectral_chroma_device(self, spec, chroma, sample_rates, d_pcm, plane_stride, channels, d_frames, d_rows, d_seg_row_off=None, stream=None):
        """vsyn_spectral_chroma_device on device pointers (ints); chroma (a SpectralChroma) may be None for the defaults."""
        rates = _rates(sample_rates)
        err = C.c_char_p()
        _check(self.lib.vsyn_spectral_chroma_device(self.h, C.byref(spec), _ref(chroma), len(rates), _ptr(rates), d_pcm, plane_stride, channels,
                                                    d_frames, d_rows, d_seg_row_off, stream, C.byref(err)), err)

    def piptrack_device(self, spec, tun, sample_rates, d_pcm, plane_stride, channels, d_frames, d_pitches, d_mags, d_seg_row_off=None, stream=None):
        """vsyn_piptrack_device on device pointers (ints); spec is a lin_power SpectralSpec, tun a TuningSpec."""
        rates = _rates(sample_rates)
        err = C.c_char_p()
        _check(self.lib.vsyn_piptrack_device(self.h, C.byref(spec), C.byref(tun), len(rates), _ptr(rates), d_pcm, plane_stride, channels, d_frames,
                                             d_pitches, d_mags, d_seg_row_off, stream, C.byref(err)), err)

    def tuning_device(self, spec, tun, sample_rates, d_pcm, plane_stride, channels, d_frames, d_tuning, d_counts, stream=None):
        """vsyn_tuning_device on device pointers (ints): d_tuning [S] float64, d_counts [S][2] uint64."""
        rates = _rates(sample_rates)
        err = C.c_char_p()
        _check(self.lib.vsyn_tuning_device(self.h, C.byref(spec), C.byref(tun), len(rates), _ptr(rates), d_pcm, plane_stride, channels, d_frames,
                                           d_tuning, d_counts, stream, C.byref(err)), err)

    def pcm_tuning_host(self, spec, tun, in_rates, out_rate=0, rows=False):
        """vsyn_pcm_tuning_host over the last submit's segments: dict(rc, tuning [S] float64, counts [S][2] uint64, seg_rows [S], flags)
        and with rows=True pitches and mags, float32 [total][NB]."""
        rates = _rates(in_rates)
        S, nb = len(rates), int(spec.n_fft) // 2 + 1
        tuning, counts, seg_rows = np.zeros(max(1, S), np.float64), np.zeros((max(1, S), 2), np.uint64), np.zeros(max(1, S), np.uint64)
        st, err = Status(), C.c_char_p()
        head = (self.h, C.byref(spec), C.byref(tun), S, _ptr(rates), out_rate)
        out = {}
        if rows:
            _check(self.lib.vsyn_pcm_tuning_host(*head, VSYN_TUNING_ROWS, None, None, None, 0, _ptr(seg_rows), C.byref(st), C.byref(err)), err)
            total = int(seg_rows[:S].sum())
            r = np.zeros((max(1, total), 2 * nb), np.float32)
            rc = self.lib.vsyn_pcm_tuning_host(*head, VSYN_TUNING_ROWS, _ptr(tuning), _ptr(counts), _ptr(r), total, _ptr(seg_rows), C.byref(st),
                                               C.byref(err))
            out = dict(pitches=r[:total, :nb], mags=r[:total, nb:])
        else:
            rc = self.lib.vsyn_pcm_tuning_host(*head, VSYN_TUNING_ONLY, _ptr(tuning), _ptr(counts), None, 0, _ptr(seg_rows), C.byref(st),
                                               C.byref(err))
        _check(rc, err, (VSYN_OK, VSYN_ERR_STREAM))
        return dict(rc=rc, tuning=tuning[:S], counts=counts[:S], seg_rows=seg_rows[:S], flags=st.flags, **out)

    def spectral_post_device(self, post, dim, seg_rows, d_in, d_out, stream=None):
        """vsyn_spectral_post_device on device pointers (ints); seg_rows is a host sequence of each segment's row count."""
        nrows = np.ascontiguousarray(seg_rows, dtype=np.uint64)
        err = C.c_char_p()
        _check(self.lib.vsyn_spectral_post_device(self.h, C.byref(post), dim, len(nrows), _ptr(nrows), d_in, d_out, stream, C.byref(err)), err)

    def pcm_spectral_post_host(self, spec, post, in_rates, out_rate=0):
        """vsyn_pcm_spectral_post_host over the last submit's segments: returns dict(rc, rows [total][D_out], seg_rows [S], flags)."""
        rates = _rates(in_rates)
        return self._rows_host(self.lib.vsyn_pcm_spectral_post_host, (C.byref(spec), C.byref(post), len(rates), _ptr(rates), out_rate), len(rates),
                               _post_dim(spec, post))

    def resample_device(self, in_rates, out_rate, d_pcm, plane_stride, channels, d_frames, d_out, out_plane_stride, d_out_frames,
                        stream=None):
        """vsyn_resample_device on device pointers (ints); in_rates is a host sequence."""
        rates = _rates(in_rates)
        err = C.c_char_p()
        _check(self.lib.vsyn_resample_device(self.h, len(rates), _ptr(rates), out_rate, d_pcm, plane_stride, channels, d_frames, d_out,
                                             out_plane_stride, d_out_frames, stream, C.byref(err)), err)

    def pcm_resample_host(self, in_rates, out_rate, fmt=VSYN_PCM_F32):
        """vsyn_pcm_resample_host over the last submit's segments: returns (pcm, frames [S]); pcm is float32 [S][C][stride] (planar)
        or int16 [S][stride][C] (interleaved), stride = the largest T_out."""
        rates = _rates(in_rates)
        return self._pcm_host(self.lib.vsyn_pcm_resample_host, (len(rates), _ptr(rates), out_rate, fmt), len(rates), fmt, self.channels,
                              lambda t_max: [])

    def pcm_condition_device(self, cond, d_pcm, plane_stride, channels, num_segments, d_frames, d_out, out_plane_stride, d_peaks=None,
                             stream=None):
        """vsyn_pcm_condition_device on device pointers (ints)."""
        err = C.c_char_p()
        _check(self.lib.vsyn_pcm_condition_device(self.h, C.byref(cond), num_segments, d_pcm, plane_stride, channels, d_frames, d_out,
                                                  out_plane_stride, d_peaks, stream, C.byref(err)), err)

    def pcm_condition_host(self, cond, num_segments, in_rates=None, out_rate=0, fmt=VSYN_PCM_F32):
        """vsyn_pcm_condition_host over the last submit's segments: returns (pcm [S][stride] float32 or int16, frames [S], peaks [S]),
        stride = the largest T."""
        S, rates, o = num_segments, _rates(in_rates), _per_segment(num_segments, "peaks")
        out, frames = self._pcm_host(self.lib.vsyn_pcm_condition_host, (C.byref(cond), S, _ptr(rates), out_rate, fmt), S, fmt, None,
                                     lambda t_max: [o["peaks"]])
        return out, frames, o["peaks"][:S]

    def pcm_cond_spectral_host(self, cond, spec, post, in_rates, out_rate=0):
        """vsyn_pcm_cond_spectral_host over the last submit's segments (cond / post may be None): returns dict(rc, rows [total][D_out],
        seg_rows [S], peaks [S], flags)."""
        rates = _rates(in_rates)
        S, o = len(rates), _per_segment(len(rates), "peaks")
        return self._rows_host(self.lib.vsyn_pcm_cond_spectral_host, (_ref(cond), C.byref(spec), _ref(post), S, _ptr(rates), out_rate), S,
                               _post_dim(spec, post), [o["peaks"]], o)

    def pcm_trim_device(self, trim, d_pcm, plane_stride, channels, num_segments, d_frames, d_out, out_plane_stride, d_out_frames, d_bounds,
                        d_ref=None, d_ms=None, ms_stride=0, stream=None):
        """vsyn_pcm_trim_device on device pointers (ints)."""
        err = C.c_char_p()
        _check(self.lib.vsyn_pcm_trim_device(self.h, _ref(trim), num_segments, d_pcm, plane_stride, channels, d_frames, d_out, out_plane_stride,
                                             d_out_frames, d_bounds, d_ref, d_ms, ms_stride, stream, C.byref(err)), err)

    def pcm_trim_host(self, trim, cond, num_segments, in_rates=None, out_rate=0, fmt=VSYN_PCM_F32):
        """vsyn_pcm_trim_host over the last submit's segments (trim / cond may be None): returns dict(pcm [S][stride] float32 or
        int16, frames [S], bounds [S][2], peaks [S], refs [S]), stride = the largest untrimmed T."""
        S, rates, o = num_segments, _rates(in_rates), _per_segment(num_segments, "bounds", "peaks", "refs")
        out, frames = self._pcm_host(self.lib.vsyn_pcm_trim_host, (_ref(trim), _ref(cond), S, _ptr(rates), out_rate, fmt), S, fmt, None,
                                     lambda t_max: [o["bounds"], o["peaks"], o["refs"]])
        return dict(pcm=out, frames=frames, **{k: v[:S] for k, v in o.items()})

    def pcm_trim_spectral_host(self, trim, cond, spec, post, in_rates, out_rate=0):
        """vsyn_pcm_trim_spectral_host over the last submit's segments (trim / cond / post may be None): returns dict(rc, rows
        [total][D_out], seg_rows [S], bounds [S][2], peaks [S], refs [S], flags)."""
        rates = _rates(in_rates)
        S, o = len(rates), _per_segment(len(rates), "bounds", "peaks", "refs")
        return self._rows_host(self.lib.vsyn_pcm_trim_spectral_host, (_ref(trim), _ref(cond), C.byref(spec), _ref(post), S, _ptr(rates), out_rate), S,
                               _post_dim(spec, post), [o["bounds"], o["peaks"], o["refs"]], o)

    def spectral_pcen_device(self, pcen, dim, seg_rows, sample_rates, hop_length, d_in, d_out, stream=None):
        """vsyn_spectral_pcen_device on device pointers (ints); seg_rows and sample_rates (None: NULL) are host sequences."""
        nrows, rates = np.ascontiguousarray(seg_rows, dtype=np.uint64), _rates(sample_rates)
        err = C.c_char_p()
        _check(self.lib.vsyn_spectral_pcen_device(self.h, _ref(pcen), dim, len(nrows), _ptr(nrows), _ptr(rates), hop_length, d_in, d_out, stream,
                                                  C.byref(err)), err)

    def spectral_hpss_device(self, hpss, dim, seg_rows, d_in, d_out, stream=None):
        """vsyn_spectral_hpss_device on device pointers (ints); seg_rows is a host sequence of each segment's row count. d_out may
        be d_in."""
        nrows = np.ascontiguousarray(seg_rows, dtype=np.uint64)
        err = C.c_char_p()
        _check(self.lib.vsyn_spectral_hpss_device(self.h, _ref(hpss), dim, len(nrows), _ptr(nrows), d_in, d_out, stream, C.byref(err)), err)

    def istft_device(self, spec, seg_rows, d_rows, d_mask, lengths, d_pcm_out, out_plane_stride, d_out_frames=None, stream=None):
        """vsyn_istft_device on device pointers (ints; d_mask and d_out_frames may be None); seg_rows and lengths (None: what each
        segment's rows cover) are host sequences."""
        nrows = np.ascontiguousarray(seg_rows, dtype=np.uint64)
        lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint64)
        err = C.c_char_p()
        _check(self.lib.vsyn_istft_device(self.h, _ref(spec), len(nrows), _ptr(nrows), d_rows, d_mask, _ptr(lens), d_pcm_out, out_plane_stride,
                                          d_out_frames, stream, C.byref(err)), err)

    def pcm_hpss_device(self, effect, frames, d_pcm, plane_stride, channels, d_pcm_out, out_plane_stride, d_out_frames=None, stream=None):
        """vsyn_pcm_hpss_device on device pointers (ints; d_out_frames may be None); frames is a host sequence of each segment's frame
        count."""
        fr = np.ascontiguousarray(frames, dtype=np.uint64)
        err = C.c_char_p()
        _check(self.lib.vsyn_pcm_hpss_device(self.h, _ref(effect), len(fr), _ptr(fr), d_pcm, plane_stride, channels, d_pcm_out, out_plane_stride,
                                             d_out_frames, stream, C.byref(err)), err)

    def phase_vocoder_device(self, spec, seg_rows, rates, d_rows, d_rows_out, stream=None):
        """vsyn_phase_vocoder_device on device pointers (ints); seg_rows and rates are host sequences. Returns each segment's rows
        out (uint64 [S])."""
        nrows, r = np.ascontiguousarray(seg_rows, dtype=np.uint64), np.ascontiguousarray(rates, dtype=np.float64)
        out = np.zeros(max(1, len(nrows)), np.uint64)
        err = C.c_char_p()
        _check(self.lib.vsyn_phase_vocoder_device(self.h, _ref(spec), len(nrows), _ptr(nrows), _ptr(r), d_rows, d_rows_out, _ptr(out), stream,
                                                  C.byref(err)), err)
        return out[:len(nrows)]

    def pcm_stretch_device(self, stretch, frames, rates, shift_from_hz, d_pcm, plane_stride, channels, d_pcm_out, out_plane_stride, d_out_frames=None,
                           stream=None):
        """vsyn_pcm_stretch_device on device pointers (ints; d_out_frames may be None); frames, rates and shift_from_hz (None without
        a shift) are host sequences."""
        fr, r = np.ascontiguousarray(frames, dtype=np.uint64), np.ascontiguousarray(rates, dtype=np.float64)
        hz = None if shift_from_hz is None else np.ascontiguousarray(shift_from_hz, dtype=np.uint32)
        err = C.c_char_p()
        _check(self.lib.vsyn_pcm_stretch_device(self.h, _ref(stretch), len(fr), _ptr(fr), _ptr(r), _ptr(hz), d_pcm, plane_stride, channels, d_pcm_out,
                                                out_plane_stride, d_out_frames, stream, C.byref(err)), err)

    def onset_strength_device(self, onset, dim, seg_rows, d_rows, d_env, stream=None):
        """vsyn_onset_strength_device on device pointers (ints); seg_rows is a host sequence of each segment's row count."""
        nrows = np.ascontiguousarray(seg_rows, dtype=np.uint64)
        err = C.c_char_p()
        _check(self.lib.vsyn_onset_strength_device(self.h, _ref(onset), dim, len(nrows), _ptr(nrows), d_rows, d_env, stream, C.byref(err)), err)

    def onset_peaks_device(self, peaks, seg_rows, sample_rates, d_env, d_onsets, d_counts, d_refused=None, stream=None):
        """vsyn_onset_peaks_device on device pointers (ints); seg_rows and sample_rates are host sequences."""
        nrows, rates = np.ascontiguousarray(seg_rows, dtype=np.uint64), _rates(sample_rates)
        err = C.c_char_p()
        _check(self.lib.vsyn_onset_peaks_device(self.h, _ref(peaks), len(nrows), _ptr(nrows), _ptr(rates), d_env, d_onsets, d_counts, d_refused, stream,
                                                C.byref(err)), err)

    def beat_track_device(self, beat, seg_rows, periods, d_env, d_beats, d_counts, d_refused=None, d_localscore=None, d_cumscore=None,
                          d_backlink=None, stream=None):
        """vsyn_beat_track_device on device pointers (ints; the last four may be None); seg_rows and periods are host sequences."""
        nrows, per = np.ascontiguousarray(seg_rows, dtype=np.uint64), np.ascontiguousarray(periods, dtype=np.uint32)
        err = C.c_char_p()
        _check(self.lib.vsyn_beat_track_device(self.h, _ref(beat), len(nrows), _ptr(nrows), _ptr(per), d_env, d_beats, d_counts, d_refused,
                                               d_localscore, d_cumscore, d_backlink, stream, C.byref(err)), err)

    def tempogram_device(self, spec, seg_rows, sample_rates, d_env, d_rows=None, d_mean=None, stream=None):
        """vsyn_tempogram_device on device pointers (ints; d_rows or d_mean may be None); seg_rows and sample_rates (None: NULL) are host
        sequences."""
        nrows, rates = np.ascontiguousarray(seg_rows, dtype=np.uint64), _rates(sample_rates)
        err = C.c_char_p()
        _check(self.lib.vsyn_tempogram_device(self.h, _ref(spec), len(nrows), _ptr(nrows), _ptr(rates), d_env, d_rows, d_mean, stream, C.byref(err)),
               err)

    def pcm_trim_spectral_pcen_host(self, trim, cond, spec, pcen, post, in_rates, out_rate=0):
        """vsyn_pcm_trim_spectral_pcen_host over the last submit's segments (trim / cond / pcen / post may be None): returns what
        pcm_trim_spectral_host returns."""
        rates = _rates(in_rates)
        S, o = len(rates), _per_segment(len(rates), "bounds", "peaks", "refs")
        return self._rows_host(self.lib.vsyn_pcm_trim_spectral_pcen_host,
                               (_ref(trim), _ref(cond), C.byref(spec), _ref(pcen), _ref(post), S, _ptr(rates), out_rate), S, _post_dim(spec, post),
                               [o["bounds"], o["peaks"], o["refs"]], o)

    def pcm_split_spectral_pcen_host(self, split, cond, spec, pcen, post, in_rates, out_rate=0):
        """vsyn_pcm_split_spectral_pcen_host over the last submit's segments (split / cond / pcen / post may be None): returns what
        pcm_split_spectral_host returns."""
        rates = _rates(in_rates)
        S, o = len(rates), _per_segment(len(rates), "frames", "counts", "peaks", "refs")
        ivs = 1 if split is None else self._split_sizes(split, S, rates if out_rate else None, out_rate)[1]
        iv = np.zeros((max(1, S), ivs, 2), np.uint32)
        r = self._rows_host(self.lib.vsyn_pcm_split_spectral_pcen_host,
                            (_ref(split), _ref(cond), C.byref(spec), _ref(pcen), _ref(post), S, _ptr(rates), out_rate), S, _post_dim(spec, post),
                            [o["frames"], o["counts"], iv, ivs, o["peaks"], o["refs"]], o)
        return dict(r, intervals=self._intervals(o["counts"], iv, S))

    def pcm_split_device(self, split, d_pcm, plane_stride, channels, num_segments, d_frames, d_out, out_plane_stride, d_out_frames, d_counts,
                         d_intervals, intervals_stride, d_ref=None, d_ms=None, ms_stride=0, stream=None):
        """vsyn_pcm_split_device on device pointers (ints)."""
        err = C.c_char_p()
        _check(self.lib.vsyn_pcm_split_device(self.h, _ref(split), num_segments, d_pcm, plane_stride, channels, d_frames, d_out, out_plane_stride,
                                              d_out_frames, d_counts, d_intervals, intervals_stride, d_ref, d_ms, ms_stride, stream, C.byref(err)), err)

    def _max_intervals(self, split, t_max):
        return 1 if split is None else max(1, int(self.lib.vsyn_pcm_split_max_intervals(C.byref(split), t_max)))

    def _split_sizes(self, split, S, rates, out_rate):
        """The unsplit frames [S] of the last submit's segments and the interval stride that holds the longest one's intervals."""
        frames = np.zeros(max(1, S), np.uint64)
        err = C.c_char_p()
        _check(self.lib.vsyn_pcm_split_intervals_host(self.h, C.byref(split), S, _ptr(rates), out_rate, _ptr(frames), None, None, 0, None,
                                                      C.byref(err)), err)
        return frames, self._max_intervals(split, int(frames[:S].max()) if S else 0)

    @staticmethod
    def _intervals(counts, iv, S):
        return [iv[g, :int(counts[g])].astype(np.int64) for g in range(S)]

    def pcm_split_intervals_host(self, split, num_segments, in_rates=None, out_rate=0):
        """vsyn_pcm_split_intervals_host over the last submit's segments: returns dict(frames [S] (unsplit), counts [S], intervals (a
        list of (n, 2) int64 arrays), refs [S])."""
        S, rates, o = num_segments, _rates(in_rates), _per_segment(num_segments, "counts", "refs")
        frames, stride = self._split_sizes(split, S, rates, out_rate)
        iv = np.zeros((max(1, S), stride, 2), np.uint32)
        err = C.c_char_p()
        _check(self.lib.vsyn_pcm_split_intervals_host(self.h, C.byref(split), S, _ptr(rates), out_rate, _ptr(frames), _ptr(o["counts"]), _ptr(iv),
                                                      stride, _ptr(o["refs"]), C.byref(err)), err)
        return dict(frames=frames[:S], counts=o["counts"][:S], intervals=self._intervals(o["counts"], iv, S), refs=o["refs"][:S])

    def pcm_split_host(self, split, cond, num_segments, in_rates=None, out_rate=0, fmt=VSYN_PCM_F32):
        """vsyn_pcm_split_host over the last submit's segments (split / cond may be None): returns dict(pcm [S][stride] float32 or
        int16, frames [S], counts [S], intervals (a list of (n, 2) int64 arrays), peaks [S], refs [S]), stride = the largest unsplit T."""
        S, rates, o = num_segments, _rates(in_rates), _per_segment(num_segments, "counts", "peaks", "refs")
        iv = []

        def outs(t_max):  # the intervals are sized once the frames are known
            ivs = self._max_intervals(split, t_max)
            iv.append(np.zeros((max(1, S), ivs, 2), np.uint32))
            return [o["counts"], iv[0], ivs, o["peaks"], o["refs"]]
        out, frames = self._pcm_host(self.lib.vsyn_pcm_split_host, (_ref(split), _ref(cond), S, _ptr(rates), out_rate, fmt), S, fmt, None, outs)
        return dict(pcm=out, frames=frames, intervals=self._intervals(o["counts"], iv[0], S), **{k: v[:S] for k, v in o.items()})

    def pcm_split_spectral_host(self, split, cond, spec, post, in_rates, out_rate=0):
        """vsyn_pcm_split_spectral_host over the last submit's segments (split / cond / post may be None): returns dict(rc, rows
        [total][D_out], seg_rows [S], frames [S], counts [S], intervals, peaks [S], refs [S], flags)."""
        rates = _rates(in_rates)
        S, o = len(rates), _per_segment(len(rates), "frames", "counts", "peaks", "refs")
        ivs = 1 if split is None else self._split_sizes(split, S, rates if out_rate else None, out_rate)[1]
        iv = np.zeros((max(1, S), ivs, 2), np.uint32)
        r = self._rows_host(self.lib.vsyn_pcm_split_spectral_host, (_ref(split), _ref(cond), C.byref(spec), _ref(post), S, _ptr(rates), out_rate), S,
                            _post_dim(spec, post), [o["frames"], o["counts"], iv, ivs, o["peaks"], o["refs"]], o)
        return dict(r, intervals=self._intervals(o["counts"], iv, S))

    def pitch_device(self, spec, sample_rates, d_pcm, plane_stride, channels, d_frames, d_rows, d_seg_row_off=None, d_refused=None, stream=None):
        """vsyn_pitch_device on device pointers (ints); sample_rates is a host sequence."""
        rates = _rates(sample_rates)
        err = C.c_char_p()
        _check(self.lib.vsyn_pitch_device(self.h, _ref(spec), len(rates), _ptr(rates), d_pcm, plane_stride, channels, d_frames, d_rows,
                                          d_seg_row_off, d_refused, stream, C.byref(err)), err)

    def pcm_pitch_host(self, spec, in_rates, out_rate=0):
        """vsyn_pcm_pitch_host over the last submit's segments: returns dict(rc, rows [total][2], seg_rows [S], refused [S], flags)."""
        rates = _rates(in_rates)
        S, o = len(rates), _per_segment(len(rates), "refused")
        return self._rows_host(self.lib.vsyn_pcm_pitch_host, (C.byref(spec), S, _ptr(rates), out_rate), S, 2, [o["refused"]], o)

    def pyin_device(self, spec, sample_rates, d_pcm, plane_stride, channels, d_frames, d_rows, d_seg_row_off=None, d_refused=None, stream=None):
        """vsyn_pyin_device on device pointers (ints); sample_rates is a host sequence."""
        rates = _rates(sample_rates)
        err = C.c_char_p()
        _check(self.lib.vsyn_pyin_device(self.h, _ref(spec), len(rates), _ptr(rates), d_pcm, plane_stride, channels, d_frames, d_rows,
                                         d_seg_row_off, d_refused, stream, C.byref(err)), err)

    def pyin_decode_device(self, spec, sample_rates, d_obs, seg_rows, d_states, stream=None):
        """vsyn_pyin_decode_device on device pointers (ints); sample_rates and seg_rows are host sequences."""
        rates, rows = _rates(sample_rates), np.ascontiguousarray(seg_rows, dtype=np.uint64)
        err = C.c_char_p()
        _check(self.lib.vsyn_pyin_decode_device(self.h, _ref(spec), len(rates), _ptr(rates), d_obs, _ptr(rows), d_states, stream, C.byref(err)), err)

    def pcm_pyin_host(self, spec, in_rates, out_rate=0):
        """vsyn_pcm_pyin_host over the last submit's segments: returns dict(rc, rows [total][3], seg_rows [S], refused [S], flags)."""
        rates = _rates(in_rates)
        S, o = len(rates), _per_segment(len(rates), "refused")
        return self._rows_host(self.lib.vsyn_pcm_pyin_host, (C.byref(spec), S, _ptr(rates), out_rate), S, 3, [o["refused"]], o)

    def fdesc_device(self, spec, sample_rates, d_pcm, plane_stride, channels, d_frames, d_rows, d_seg_row_off=None, d_refused=None, stream=None):
        """vsyn_fdesc_device on device pointers (ints); sample_rates is a host sequence (None: NULL)."""
        rates = _rates(sample_rates)
        err = C.c_char_p()
        _check(self.lib.vsyn_fdesc_device(self.h, _ref(spec), 0 if rates is None else len(rates), _ptr(rates), d_pcm, plane_stride, channels,
                                          d_frames, d_rows, d_seg_row_off, d_refused, stream, C.byref(err)), err)

    def pcm_fdesc_host(self, spec, in_rates, out_rate=0):
        """vsyn_pcm_fdesc_host over the last submit's segments: returns dict(rc, rows [total][6], seg_rows [S], refused [S], flags)."""
        rates = _rates(in_rates)
        S, o = len(rates), _per_segment(len(rates), "refused")
        return self._rows_host(self.lib.vsyn_pcm_fdesc_host, (C.byref(spec), S, _ptr(rates), out_rate), S, 6, [o["refused"]], o)

    def cqt_device(self, spec, sample_rates, d_pcm, plane_stride, channels, d_frames, d_rows, d_seg_row_off=None, d_refused=None, stream=None):
        """vsyn_cqt_device on device pointers (ints); sample_rates is a host sequence (None: NULL)."""
        rates = _rates(sample_rates)
        err = C.c_char_p()
        _check(self.lib.vsyn_cqt_device(self.h, _ref(spec), 0 if rates is None else len(rates), _ptr(rates), d_pcm, plane_stride, channels,
                                        d_frames, d_rows, d_seg_row_off, d_refused, stream, C.byref(err)), err)

    def pcm_cqt_host(self, spec, in_rates, out_rate=0):
        """vsyn_pcm_cqt_host over the last submit's segments: returns dict(rc, rows [total][dim], seg_rows [S], refused [S], flags)."""
        rates = _rates(in_rates)
        S, o = len(rates), _per_segment(len(rates), "refused")
        dim = int(self.lib.vsyn_cqt_dim(C.byref(spec)))
        return self._rows_host(self.lib.vsyn_pcm_cqt_host, (C.byref(spec), S, _ptr(rates), out_rate), S, max(dim, 1), [o["refused"]], o)

    def pcm_cqt_est_host(self, spec, estimate, in_rates, out_rate=0):
        """vsyn_pcm_cqt_est_host over the last submit's segments: what pcm_cqt_host returns and tuning [S] float64 (estimate: a
        TuningSpec, or None for pcm_cqt_host itself: tuning stays zeros)."""
        rates = _rates(in_rates)
        S, o = len(rates), _per_segment(len(rates), "refused")
        dim, tun = int(self.lib.vsyn_cqt_dim(C.byref(spec))), np.zeros(max(1, len(rates)), np.float64)
        r = self._rows_host(self.lib.vsyn_pcm_cqt_est_host, (C.byref(spec), _ref(estimate), S, _ptr(rates), out_rate), S, max(dim, 1),
                            [o["refused"], tun], o)
        return dict(r, tuning=tun[:S])

    def loudness_device(self, spec, sample_rates, frames, d_pcm, plane_stride, channels, d_records, d_z=None, d_weighted=None,
                        weighted_plane_stride=0, d_scaled=None, scaled_plane_stride=0, stream=None):
        """vsyn_loudness_device on device pointers (ints); sample_rates and frames are host sequences."""
        rates, fr = _rates(sample_rates), np.ascontiguousarray(frames, dtype=np.uint64)
        err = C.c_char_p()
        _check(self.lib.vsyn_loudness_device(self.h, _ref(spec), len(rates), _ptr(rates), _ptr(fr), d_pcm, plane_stride, channels, d_records, d_z,
                                             d_weighted, weighted_plane_stride, d_scaled, scaled_plane_stride, stream, C.byref(err)), err)

    def pcm_loudness_host(self, spec, in_rates, out_rate=0, blocks=False):
        """vsyn_pcm_loudness_host over the last submit's segments: returns dict(rc, records [S] (LOUDNESS_RECORD_DTYPE), seg_blocks [S],
        z (blocks=True: the block means back to back, else None), flags)."""
        rates = _rates(in_rates)
        S = len(rates)
        rec, nb = np.zeros(max(1, S), LOUDNESS_RECORD_DTYPE), np.zeros(max(1, S), np.uint64)
        st, err = Status(), C.c_char_p()
        head = (self.h, _ref(spec), S, _ptr(rates), out_rate)
        z = None
        if blocks:  # the size query first: nothing is launched for NULL records
            _check(self.lib.vsyn_pcm_loudness_host(*head, None, None, 0, _ptr(nb), C.byref(st), C.byref(err)), err)
            z = np.zeros(max(1, int(nb[:S].sum())), np.float64)
        rc = self.lib.vsyn_pcm_loudness_host(*head, _ptr(rec), _ptr(z), 0 if z is None else len(z), _ptr(nb), C.byref(st), C.byref(err))
        _check(rc, err, (VSYN_OK, VSYN_ERR_STREAM))
        return dict(rc=rc, records=rec[:S], seg_blocks=nb[:S], z=None if z is None else z[:int(nb[:S].sum())], flags=st.flags)

    def _chain_pcm_host(self, fn, gate, gate_is_split, stages, cond, num_segments, in_rates, out_rate, fmt):
        """The PCM chain entries: stages are the arguments between gate_is_split and cond, as fn takes them."""
        S, rates, o = num_segments, _rates(in_rates), _per_segment(num_segments, "bounds", "counts", "peaks", "refs")
        rec, iv = np.zeros(max(1, S), LOUDNESS_RECORD_DTYPE), []

        def outs(t_max):
            ivs = self._max_intervals(gate, t_max) if gate is not None and gate_is_split else 1
            iv.append(np.zeros((max(1, S), ivs, 2), np.uint32))
            return [o["bounds"], o["counts"], iv[0], ivs, o["peaks"], o["refs"], rec]
        out, frames = self._pcm_host(fn, (_ref(gate), 1 if gate_is_split else 0, *stages, _ref(cond), S, _ptr(rates), out_rate, fmt), S, fmt, None, outs)
        return dict(pcm=out, frames=frames, intervals=self._intervals(o["counts"], iv[0], S), records=rec[:S], **{k: v[:S] for k, v in o.items()})

    def pcm_chain_host(self, gate, gate_is_split, loud, cond, num_segments, in_rates=None, out_rate=0, fmt=VSYN_PCM_F32):
        """vsyn_pcm_chain_host over the last submit's segments (gate / loud / cond may be None, but not all three): returns dict(pcm
        [S][stride], frames [S], bounds [S][2], counts [S], intervals, peaks [S], refs [S], records [S])."""
        return self._chain_pcm_host(self.lib.vsyn_pcm_chain_host, gate, gate_is_split, (_ref(loud),), cond, num_segments, in_rates, out_rate, fmt)

    def pcm_chain_effects_host(self, gate, gate_is_split, effect, loud, cond, num_segments, in_rates=None, out_rate=0, fmt=VSYN_PCM_F32):
        """vsyn_pcm_chain_effects_host over the last submit's segments (every spec may be None, but not all four): returns what
        pcm_chain_host returns."""
        return self._chain_pcm_host(self.lib.vsyn_pcm_chain_effects_host, gate, gate_is_split, (_ref(effect), _ref(loud)), cond, num_segments,
                                    in_rates, out_rate, fmt)

    def pcm_chain_stretch_host(self, gate, gate_is_split, effect, stretch, stretch_rates, shift_from_hz, loud, cond, num_segments, in_rates=None,
                               out_rate=0, fmt=VSYN_PCM_F32):
        """vsyn_pcm_chain_stretch_host over the last submit's segments (stretch_rates: one float per segment; shift_from_hz: None
        without a shift): returns what pcm_chain_host returns, frames being what the stretch delivers and the stride the largest
        length on the way."""
        sr = None if stretch_rates is None else np.ascontiguousarray(stretch_rates, dtype=np.float64)
        hz = None if shift_from_hz is None else np.ascontiguousarray(shift_from_hz, dtype=np.uint32)
        return self._chain_pcm_host(self.lib.vsyn_pcm_chain_stretch_host, gate, gate_is_split,
                                    (_ref(effect), _ref(stretch), _ptr(sr), _ptr(hz), _ref(loud)), cond, num_segments, in_rates, out_rate, fmt)

    def pcm_chain_spectral_host(self, gate, gate_is_split, loud, cond, spec, pcen, post, in_rates, out_rate=0):
        """vsyn_pcm_chain_spectral_host over the last submit's segments (gate / loud / cond / pcen / post may be None): returns what
        pcm_split_spectral_host returns, with bounds [S][2] and records [S]."""
        rates = _rates(in_rates)
        S, o = len(rates), _per_segment(len(rates), "frames", "bounds", "counts", "peaks", "refs")
        rec = np.zeros(max(1, S), LOUDNESS_RECORD_DTYPE)
        ivs = self._split_sizes(gate, S, rates if out_rate else None, out_rate)[1] if gate is not None and gate_is_split else 1
        iv = np.zeros((max(1, S), ivs, 2), np.uint32)
        r = self._rows_host(self.lib.vsyn_pcm_chain_spectral_host,
                            (_ref(gate), 1 if gate_is_split else 0, _ref(loud), _ref(cond), C.byref(spec), _ref(pcen), _ref(post), S, _ptr(rates),
                             out_rate), S, _post_dim(spec, post), [o["frames"], o["bounds"], o["counts"], iv, ivs, o["peaks"], o["refs"], rec], o)
        return dict(r, intervals=self._intervals(o["counts"], iv, S), records=rec[:S])

    def _chain_rows_host(self, fn, gate, gate_is_split, loud, cond, spec, chroma, stages, post, in_rates, out_rate):
        """The chain entries that take the chroma parameters: stages are the row stages' specs between chroma and post."""
        rates = _rates(in_rates)
        S, o = len(rates), _per_segment(len(rates), "frames", "bounds", "counts", "peaks", "refs")
        rec = np.zeros(max(1, S), LOUDNESS_RECORD_DTYPE)
        ivs = self._split_sizes(gate, S, rates if out_rate else None, out_rate)[1] if gate is not None and gate_is_split else 1
        iv = np.zeros((max(1, S), ivs, 2), np.uint32)
        r = self._rows_host(fn, (_ref(gate), 1 if gate_is_split else 0, _ref(loud), _ref(cond), C.byref(spec), _ref(chroma)) +
                            tuple(_ref(st) for st in stages) + (_ref(post), S, _ptr(rates), out_rate), S, _post_dim(spec, post, chroma),
                            [o["frames"], o["bounds"], o["counts"], iv, ivs, o["peaks"], o["refs"], rec], o)
        return dict(r, intervals=self._intervals(o["counts"], iv, S), records=rec[:S])

    def pcm_chain_chroma_est_host(self, gate, gate_is_split, loud, cond, spec, chroma, pcen, post, estimate, in_rates, out_rate=0):
        """vsyn_pcm_chain_chroma_est_host over the last submit's segments: what pcm_chain_chroma_host returns and tuning [S] float64, each
        segment's estimate (estimate: a TuningSpec, or None for pcm_chain_chroma_host itself: tuning stays zeros)."""
        rates = _rates(in_rates)
        S, o = len(rates), _per_segment(len(rates), "frames", "bounds", "counts", "peaks", "refs")
        rec, tun = np.zeros(max(1, S), LOUDNESS_RECORD_DTYPE), np.zeros(max(1, S), np.float64)
        ivs = self._split_sizes(gate, S, rates if out_rate else None, out_rate)[1] if gate is not None and gate_is_split else 1
        iv = np.zeros((max(1, S), ivs, 2), np.uint32)
        r = self._rows_host(self.lib.vsyn_pcm_chain_chroma_est_host,
                            (_ref(gate), 1 if gate_is_split else 0, _ref(loud), _ref(cond), C.byref(spec), _ref(chroma), _ref(pcen), _ref(post),
                             _ref(estimate), S, _ptr(rates), out_rate), S, _post_dim(spec, post, chroma),
                            [o["frames"], o["bounds"], o["counts"], iv, ivs, o["peaks"], o["refs"], rec, tun], o)
        return dict(r, intervals=self._intervals(o["counts"], iv, S), records=rec[:S], tuning=tun[:S])

    def pcm_chain_chroma_host(self, gate, gate_is_split, loud, cond, spec, chroma, pcen, post, in_rates, out_rate=0):
        """vsyn_pcm_chain_chroma_host over the last submit's segments (every spec but spec may be None): returns what
        pcm_chain_spectral_host returns."""
        return self._chain_rows_host(self.lib.vsyn_pcm_chain_chroma_host, gate, gate_is_split, loud, cond, spec, chroma, (pcen,), post, in_rates,
                                     out_rate)

    def pcm_chain_hpss_host(self, gate, gate_is_split, loud, cond, spec, chroma, hpss, pcen, post, in_rates, out_rate=0):
        """vsyn_pcm_chain_hpss_host over the last submit's segments (every spec but spec may be None): returns what
        pcm_chain_spectral_host returns."""
        return self._chain_rows_host(self.lib.vsyn_pcm_chain_hpss_host, gate, gate_is_split, loud, cond, spec, chroma, (hpss, pcen), post,
                                     in_rates, out_rate)

    def pcm_chain_rhythm_host(self, gate, gate_is_split, loud, cond, spec, chroma, hpss, pcen, post, rhythm, in_rates, out_rate=0):
        """vsyn_pcm_chain_rhythm_host over the last submit's segments (every spec but spec may be None). rhythm None: what
        pcm_chain_hpss_host returns. Otherwise rows holds the selected output's words as float32 [rows][columns] (1 column for the
        envelope and, to be viewed as uint32, the onsets; win_length for the tempogram; 2 for the mean's float64 values and the rate
        behind them), seg_rows its rows per segment, and refused [S] the refusal words."""
        rates = _rates(in_rates)
        S, o = len(rates), _per_segment(len(rates), "frames", "bounds", "counts", "peaks", "refs", "refused")
        rec = np.zeros(max(1, S), LOUDNESS_RECORD_DTYPE)
        ivs = self._split_sizes(gate, S, rates if out_rate else None, out_rate)[1] if gate is not None and gate_is_split else 1
        iv = np.zeros((max(1, S), ivs, 2), np.uint32)
        fn = self.lib.vsyn_pcm_chain_rhythm_host
        head = (_ref(gate), 1 if gate_is_split else 0, _ref(loud), _ref(cond), C.byref(spec), _ref(chroma), _ref(hpss), _ref(pcen), _ref(post),
                _ref(rhythm), S, _ptr(rates), out_rate)
        outs = [o["frames"], o["bounds"], o["counts"], iv, ivs, o["peaks"], o["refs"], rec, o["refused"]]
        if rhythm is None:
            r = self._rows_host(fn, head, S, _post_dim(spec, post, chroma), outs, o)
        else:
            cols = {2: rhythm.tempogram.win_length, 3: 2}.get(rhythm.output, 1)
            seg_rows, st = np.zeros(max(1, S), np.uint64), Status()

            def alloc():  # the first call counted the spectral rows: F words a segment (F win_length for the tempogram), 4098 for a mean
                words = int(seg_rows[:S].sum()) * max(cols, 1) + 4098 * S + 1
                return np.zeros(words, np.float32), words, outs
            rc, buf = self._sized_call(fn, head, seg_rows, alloc, st, (VSYN_OK, VSYN_ERR_STREAM))
            n = int(seg_rows[:S].sum())
            r = dict(rc=rc, rows=buf[:n * cols].reshape(n, cols), seg_rows=seg_rows[:S], flags=st.flags, **{k: v[:S] for k, v in o.items()})
        return dict(r, intervals=self._intervals(o["counts"], iv, S), records=rec[:S])

    def attach_vq(self, vq_spec):
        """vsyn_attach_vq: codebook value tables + residue descriptions for the device VQ stage."""
        self._vq = vq_spec.c_setup()
        err = C.c_char_p()
        _check(self.lib.vsyn_attach_vq(self.h, C.byref(self._vq), C.byref(err)), err)
        self.fused_paths = self.lib.vsyn_fused_paths(self.h)  # (+ bit 8: the VQ kernel keeps this setup's value tables in LDS)

    def submit_host_vq(self, packets, segments, ys, vq_packets, cls, entries, residue_floats, plane_stride,
                       want_residue=True, flags=0):
        """Like submit_host with the residue given as classification + entry numbers; returns 'residue' (the
        rebuilt after_residue tensor) when want_residue."""
        P, S, Cn = len(packets), len(segments), self.channels
        packets = np.ascontiguousarray(packets, dtype=PACKET_DTYPE)
        segments = np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE)
        ys = np.ascontiguousarray(ys, dtype=np.uint16)
        vq_packets = np.ascontiguousarray(vq_packets, dtype=VQ_PACKET_DTYPE)
        cls = np.ascontiguousarray(cls, dtype=np.uint8)
        entries = np.ascontiguousarray(entries, dtype=np.uint16)
        pcm = np.zeros((S, Cn, plane_stride), np.float32)
        emit = np.zeros(P, np.uint32)
        res = np.zeros(residue_floats, np.float32) if want_residue else None
        vb = VqBatch(vq_packets.ctypes.data, cls.ctypes.data if cls.size else None,
                     entries.ctypes.data if entries.size else None, cls.size, entries.size)
        st, err = Status(), C.c_char_p()
        rc = self.lib.vsyn_submit_host_vq(self.h, P, _ptr(packets), S, _ptr(segments), _ptr(ys), C.byref(vb), _ptr(res),
                                          residue_floats, _ptr(pcm), plane_stride, _ptr(emit), None, flags,
                                          C.byref(st), C.byref(err))
        _check(rc, err, (VSYN_OK, VSYN_ERR_STREAM))
        return dict(rc=rc, pcm=pcm, emit_len=emit, residue=res, flags=st.flags, first_bad=st.first_bad_packet)

    def submit_device_vq(self, P, d_packets, S, d_segments, max_seg_packets, d_ys, d_vq_packets, d_cls, num_cls, d_entries,
                         num_entries, d_residue, d_pcm, plane_stride, d_emit=None, flags=0, stream=None):
        """All pointers are raw device addresses (ints)."""
        err = C.c_char_p()
        vb = VqBatch(d_vq_packets, d_cls, d_entries, num_cls, num_entries)
        _check(self.lib.vsyn_submit_device_vq(self.h, P, d_packets, S, d_segments, max_seg_packets, d_ys, C.byref(vb),
                                              d_residue, d_pcm, plane_stride, d_emit, None, flags, stream, C.byref(err)), err)

    def submit_device(self, P, d_packets, S, d_segments, max_seg_packets, d_ys, d_residue, d_pcm, plane_stride,
                      d_emit=None, taps=None, flags=0, stream=None):
        """All arguments are raw device addresses (ints)."""
        err = C.c_char_p()
        tp = C.byref(Taps(*taps)) if taps else None
        _check(self.lib.vsyn_submit_device(self.h, P, d_packets, S, d_segments, max_seg_packets, d_ys, d_residue,
                                           d_pcm, plane_stride, d_emit, tp, flags, stream, C.byref(err)), err)

    def pcm_interleave_device(self, fmt, d_pcm, plane_stride, d_out, out_stride_frames, d_frames=None, stream=None):
        """Interleave / convert the PCM of the most recent submit_device* (raw device addresses)."""
        err = C.c_char_p()
        _check(self.lib.vsyn_pcm_interleave_device(self.h, fmt, d_pcm, plane_stride, d_out, out_stride_frames, d_frames, stream,
                                                   C.byref(err)), err)

    def pcm_fetch_host(self, fmt, num_segments, out_stride_frames):
        """The PCM of the most recent submit_host*, converted on the device -> ([S][out_stride_frames][C] int16 / float32, frames [S])."""
        out = np.zeros((num_segments, out_stride_frames, self.channels), np.int16 if fmt == VSYN_PCM_S16 else np.float32)
        frames = np.zeros(num_segments, np.uint32)
        err = C.c_char_p()
        _check(self.lib.vsyn_pcm_fetch_host(self.h, fmt, out.ctypes.data, out_stride_frames, frames.ctypes.data, C.byref(err)), err)
        return out, frames

    def pcm_abs_sum_host(self, num_segments):
        """Per-(segment, channel) sum |x| of the PCM of the most recent submit_host*, computed on the device -> [S][C] float64."""
        out = np.zeros((num_segments, self.channels), np.float64)
        err = C.c_char_p()
        _check(self.lib.vsyn_pcm_abs_sum_host(self.h, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(err)), err)
        return out

    def sync_status(self, stream=None):
        st, err = Status(), C.c_char_p()
        _check(self.lib.vsyn_sync_status(self.h, stream, C.byref(st), C.byref(err)), err, (VSYN_OK, VSYN_ERR_STREAM))
        return st.flags, st.first_bad_packet

    def imdct_device(self, n, count, d_in, d_out, stream=None):
        err = C.c_char_p()
        _check(self.lib.vsyn_imdct_device(self.h, n, count, d_in, d_out, stream, C.byref(err)), err)

    def profile(self, on=1):
        """0/False off, 1/True long-run fused kernel, 2 mixed-block fused kernel."""
        self.lib.vsyn_profile_enable(self.h, int(on))

    def profile_read(self):
        ms, n, name = C.c_double(), C.c_uint32(), C.c_char_p()
        self.lib.vsyn_profile_read(self.h, C.byref(ms), C.byref(n), C.byref(name))
        return ms.value, n.value, (name.value or b"").decode()
