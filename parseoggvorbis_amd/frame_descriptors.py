"""Per-frame energy, zero-crossing rate and spectral shape from Ogg bytes, computed on the GPU: a list of (rows (F, 6), sr). ctypes onto
libparseoggvorbis_amd.so (ogg_vorbis_fdesc_corpus). The columns are COLUMNS: rms, zcr, centroid, bandwidth, rolloff, flatness, as
librosa.feature.rms / zero_crossing_rate / spectral_centroid / spectral_bandwidth / spectral_rolloff / spectral_flatness define them
on the mono signal y = get_pcm_batch(mono=True, sr=sr), after the optional resampler and before anything is copied back: no PCM
crosses the bus. The arithmetic is written out in include/vorbis_synth_hip.h ("frame descriptors") and the float64 model in
tests/fdesc_model.py is the contract; parity with librosa itself is not claimed. Row f lines up with row f of
get_spectral_batch(n_fft=n_fft, hop_length=hop_length, center=center) and with frame f of get_f0_batch(frame_length=n_fft,
hop_length=hop_length, center=center).

Every argument is checked before the library is loaded."""
import ctypes as C
import math

import numpy as np

from . import _corpus
from ._corpus import HOST_LIB_PATH  # noqa: F401
from .pcm import TRIM_MAX_FRAME, U32_MAX, check_sr

COLUMNS = ("rms", "zcr", "centroid", "bandwidth", "rolloff", "flatness")
FDESC_CENTER = 1  # VSYN_FDESC_CENTER
MIN_FFT = 16


class FrameDescriptorError(RuntimeError):
    pass


def _real(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise FrameDescriptorError("%s must be a number, got %r" % (name, v))
    if not math.isfinite(float(v)):
        raise FrameDescriptorError("%s must be finite, got %r" % (name, v))
    return float(v)


def _int(name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise FrameDescriptorError("%s must be an integer, got %r" % (name, v))
    if not lo <= int(v) <= hi:
        raise FrameDescriptorError("%s must be in [%d, %d], got %d" % (name, lo, hi, int(v)))
    return int(v)


def fdesc_spec(n_fft=2048, hop_length=512, win_length=None, center=True, roll_percent=0.85, zcr_threshold=1e-10, amin=1e-10):
    """Checks the arguments (include/vorbis_synth_hip.h, "frame descriptors", step 11) and returns the C spec (binding.FdescSpec):
    n_fft an integer in [16, 8192]; hop_length an integer >= 1 (that the C spec's uint32 holds); win_length None (n_fft) or an
    integer in [1, n_fft]; center a bool; 0 < roll_percent < 1; zcr_threshold >= 0 and amin > 0, finite."""
    from .binding import FdescSpec
    n = _int("n_fft", n_fft, MIN_FFT, TRIM_MAX_FRAME)
    hop = _int("hop_length", hop_length, 1, U32_MAX)
    win = n if win_length is None else _int("win_length", win_length, 1, n)
    if not isinstance(center, (bool, np.bool_)):
        raise FrameDescriptorError("center must be a bool, got %r" % (center,))
    roll, thr, am = _real("roll_percent", roll_percent), _real("zcr_threshold", zcr_threshold), _real("amin", amin)
    if not 0.0 < roll < 1.0:
        raise FrameDescriptorError("roll_percent must be in (0, 1), got %r" % (roll_percent,))
    if not thr >= 0.0:
        raise FrameDescriptorError("zcr_threshold must be >= 0, got %r" % (zcr_threshold,))
    if not am > 0.0:
        raise FrameDescriptorError("amin must be > 0, got %r" % (amin,))
    return FdescSpec(n, hop, win, FDESC_CENTER if center else 0, roll, thr, am)


_load = _corpus.load


def get_frame_descriptors_batch(list_of_bytes, n_fft=2048, hop_length=512, win_length=None, center=True, roll_percent=0.85,
                                zcr_threshold=1e-10, amin=1e-10, sr=None, threads=0, feeders=0, device=0, errors="raise",
                                files_per_submit=64, stats=None):
    """The frame descriptors of many Ogg Vorbis files in one corpus run: a list of (rows, sr) tuples. rows is float32 (F, 6), the
    columns COLUMNS; sr is the rate they were computed at (centroid, bandwidth and rolloff are in Hz at that rate). sr, threads,
    feeders, errors and stats as for get_pcm_batch. A file with an Inf or NaN sample fails alone: errors="raise" raises
    FrameDescriptorError naming the first such file, errors="return" puts the FrameDescriptorError in its slot."""
    if errors not in ("raise", "return"):
        raise FrameDescriptorError("errors must be 'raise' or 'return', got %r" % (errors,))
    target = check_sr(sr, FrameDescriptorError)
    spec = fdesc_spec(n_fft, hop_length, win_length, center, roll_percent, zcr_threshold, amin)
    threads, feeders = _int("threads", threads, 0, 1 << 16), _int("feeders", feeders, 0, 1 << 16)
    device, files_per_submit = _int("device", device, 0, 1 << 16), _int("files_per_submit", files_per_submit, 1, 65535)
    lib = _load()
    n = len(list_of_bytes)
    counts = np.zeros(max(n, 1), np.uint64)
    frames = np.zeros(max(n, 1), np.uint64)
    rates = np.zeros(max(n, 1), np.uint32)

    def build(i, p):
        return _corpus.copy_into(np.zeros((int(counts[i]), len(COLUMNS)), np.float32), p), int(rates[i])

    return _corpus.run(lib, lib.ogg_vorbis_fdesc_corpus, list_of_bytes, (threads, feeders, files_per_submit, device, target, C.byref(spec)),
                       (counts, frames, rates), build, FrameDescriptorError, errors, "frame descriptor", stats)


def get_frame_descriptors_from_raw_bytes(raw_bytes, **kwargs):
    """One file's (rows, sr), as get_frame_descriptors_batch."""
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return get_frame_descriptors_batch([raw_bytes], **kwargs)[0]
