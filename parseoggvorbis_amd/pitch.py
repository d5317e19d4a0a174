"""Fundamental frequency per frame from Ogg bytes, estimated on the GPU: a list of (f0, cmnd, sr). ctypes onto
libparseoggvorbis_amd.so (ogg_vorbis_pitch_corpus). The estimator is YIN as librosa.yin computes it (librosa >= 0.10 defaults:
win_length = frame_length // 2, pad_mode="constant") on the mono signal y = get_pcm_batch(mono=True, sr=sr), after the optional
resampler and before anything is copied back: no PCM crosses the bus. The arithmetic is written out in include/vorbis_synth_hip.h
("pitch") and the float64 model in tests/pitch_model.py is the contract; parity with librosa itself is not claimed. Frame f lines
up with row f of get_spectral_batch(n_fft=frame_length, hop_length=hop_length).

Every argument is checked before the library is loaded."""
import ctypes as C
import math

import numpy as np

from . import _corpus
from ._corpus import HOST_LIB_PATH  # noqa: F401
from .pcm import TRIM_MAX_FRAME, U32_MAX, check_sr

PITCH_CENTER = 1  # VSYN_PITCH_CENTER
MIN_FRAME = 4


class PitchError(RuntimeError):
    pass


def _real(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise PitchError("%s must be a number, got %r" % (name, v))
    if not math.isfinite(float(v)):
        raise PitchError("%s must be finite, got %r" % (name, v))
    return float(v)


def pitch_spec(fmin, fmax, frame_length=2048, hop_length=None, trough_threshold=0.1, center=True):
    """Checks the arguments (include/vorbis_synth_hip.h, "pitch", step 10, as far as they can be without a file's rate) and returns
    the C spec (binding.PitchSpec): frame_length an integer in [4, 8192]; hop_length None (frame_length // 4) or an integer >= 1
    (that the C spec's uint32 holds); 0 < fmin < fmax, finite; 0 < trough_threshold <= 1; center a bool."""
    from .binding import PitchSpec
    for name, v, lo, hi in (("frame_length", frame_length, MIN_FRAME, TRIM_MAX_FRAME), ("hop_length", hop_length, 1, U32_MAX)):
        if name == "hop_length" and v is None:
            continue
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise PitchError("%s must be an integer, got %r" % (name, v))
        if not lo <= int(v) <= hi:
            raise PitchError("%s must be in [%d, %d], got %d" % (name, lo, hi, int(v)))
    if not isinstance(center, (bool, np.bool_)):
        raise PitchError("center must be a bool, got %r" % (center,))
    lo, hi, thr = _real("fmin", fmin), _real("fmax", fmax), _real("trough_threshold", trough_threshold)
    if not 0.0 < lo < hi:
        raise PitchError("need 0 < fmin < fmax, got fmin %r, fmax %r" % (fmin, fmax))
    if not 0.0 < thr <= 1.0:
        raise PitchError("trough_threshold must be in (0, 1], got %r" % (trough_threshold,))
    L = int(frame_length)
    H = L // 4 if hop_length is None else int(hop_length)
    return PitchSpec(L, H, PITCH_CENTER if center else 0, 0, lo, hi, thr)


_load = _corpus.load


def get_f0_batch(list_of_bytes, fmin, fmax, frame_length=2048, hop_length=None, trough_threshold=0.1, center=True, sr=None, threads=0,
                 feeders=0, device=0, errors="raise", files_per_submit=64, stats=None):
    """The fundamental frequency of many Ogg Vorbis files in one corpus run: a list of (f0, cmnd, sr) tuples. f0 is float32 (F,), in
    Hz, what librosa.yin(y, fmin=fmin, fmax=fmax, sr=sr, frame_length=frame_length, hop_length=hop_length,
    trough_threshold=trough_threshold, center=center) computes for the mono signal y = get_pcm_batch(mono=True, sr=sr); cmnd is
    float32 (F,), the cumulative-mean-normalised difference at the chosen lag (small: periodic; near 1: not), which librosa
    discards and a caller thresholds for voicing; sr is the rate both were computed at. hop_length=None means frame_length // 4.
    sr, errors and stats as for get_pcm_batch. A file whose rate does not fit (fmax above sr / 2, or fewer than two lags between
    sr / fmax and min(sr / fmin, frame_length - frame_length // 2 - 1)) fails alone, and so does a file with an Inf or NaN sample:
    errors="raise" raises PitchError naming the first such file, errors="return" puts the PitchError in its slot."""
    _corpus.check_errors(errors)
    target = check_sr(sr, PitchError)
    spec = pitch_spec(fmin, fmax, frame_length, hop_length, trough_threshold, center)
    lib = _load()
    n = len(list_of_bytes)
    counts = np.zeros(max(n, 1), np.uint64)
    frames = np.zeros(max(n, 1), np.uint64)
    rates = np.zeros(max(n, 1), np.uint32)

    def build(i, p):
        rows = _corpus.copy_into(np.zeros((int(counts[i]), 2), np.float32), p)
        return np.ascontiguousarray(rows[:, 0]), np.ascontiguousarray(rows[:, 1]), int(rates[i])

    return _corpus.run(lib, lib.ogg_vorbis_pitch_corpus, list_of_bytes, (threads, feeders, files_per_submit, device, target, C.byref(spec)),
                       (counts, frames, rates), build, PitchError, errors, "pitch", stats)


def get_f0_from_raw_bytes(raw_bytes, fmin, fmax, **kwargs):
    """One file's (f0, cmnd, sr), as get_f0_batch."""
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return get_f0_batch([raw_bytes], fmin, fmax, **kwargs)[0]
