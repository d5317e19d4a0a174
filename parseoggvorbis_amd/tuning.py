"""Tuning estimation from Ogg bytes, computed on the GPU: librosa.piptrack's peaks behind the STFT the linear spectra compute, and
librosa.estimate_tuning / pitch_tuning per file on them, from the decoded PCM while it is still on the device (no PCM crosses the
bus). ctypes onto libparseoggvorbis_amd.so (ogg_vorbis_tuning_corpus). The arithmetic is written out in include/vorbis_synth_hip.h
("tuning estimation") and the model in tests/tuning_model.py is the contract; parity with librosa itself is not claimed.

The tuning is in fractions of a bin of bins_per_octave: the number that get_spectral_batch(kind="chroma", tuning=..., n_chroma =
bins_per_octave) and get_cqt_batch(tuning=..., bins_per_octave=...) take, and the one their tuning="estimate" computes per file with
this stage. The defaults are librosa.estimate_tuning's; librosa's chroma_stft hands the estimator its power spectrogram (power=2) at
its own framing, and its cqt a magnitude STFT of n_fft 2048 and hop 512 (power=1): those are what tuning="estimate" uses there.

Every argument is checked before the library is loaded."""
import ctypes as C
import math

import numpy as np

from . import _corpus
from ._corpus import HOST_LIB_PATH  # noqa: F401
from .pcm import check_sr

MAX_BINS = 4096  # histogram bins: ceil(1 / resolution)


class TuningError(RuntimeError):
    pass


def _real(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise TuningError("%s must be a number, got %r" % (name, v))
    if not math.isfinite(float(v)):
        raise TuningError("%s must be finite, got %r" % (name, v))
    return float(v)


def _int(name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise TuningError("%s must be an integer, got %r" % (name, v))
    if not lo <= int(v) <= hi:
        raise TuningError("%s must be in [%d, %d], got %d" % (name, lo, hi, int(v)))
    return int(v)


def tuning_spec(fmin=150.0, fmax=4000.0, threshold=0.1, resolution=0.01, bins_per_octave=12):
    """Checks the estimator's arguments (include/vorbis_synth_hip.h, "tuning estimation", step 9) and returns the C struct
    (binding.TuningSpec): fmin and fmax finite with fmax > max(fmin, 0); threshold finite and >= 0; resolution finite, inside (0, 1)
    and of at most 4096 histogram bins; bins_per_octave an integer in [1, 256]."""
    from .binding import TuningSpec
    lo, hi, thr, res = _real("fmin", fmin), _real("fmax", fmax), _real("threshold", threshold), _real("resolution", resolution)
    if not hi > max(lo, 0.0):
        raise TuningError("fmax must be above max(fmin, 0) = %g, got %r" % (max(lo, 0.0), fmax))
    if not thr >= 0.0:
        raise TuningError("threshold must be >= 0, got %r" % (threshold,))
    if not 0.0 < res < 1.0:
        raise TuningError("resolution must be inside (0, 1), got %r" % (resolution,))
    if math.ceil(1.0 / res) > MAX_BINS:
        raise TuningError("resolution %r needs more than %d histogram bins" % (resolution, MAX_BINS))
    return TuningSpec(lo, hi, thr, res, _int("bins_per_octave", bins_per_octave, 1, 256), 0)


def framing_spec(n_fft=2048, hop_length=None, win_length=None, center=True, power=1):
    """The lin_power spec (binding.SpectralSpec) of the estimator's STFT; hop_length=None means n_fft // 4."""
    from .spectral import SpectralError, spectral_spec
    if not isinstance(center, (bool, np.bool_)):
        raise TuningError("center must be a bool, got %r" % (center,))
    if hop_length is None and isinstance(n_fft, (int, np.integer)) and not isinstance(n_fft, bool):
        hop_length = max(int(n_fft) // 4, 1)  # (an n_fft that is no integer is spectral_spec's to refuse)
    try:
        return spectral_spec("lin_power", n_fft=n_fft, hop_length=hop_length, win_length=win_length, center=bool(center), power=power)
    except SpectralError as e:
        raise TuningError(str(e)) from None


_load = _corpus.load


def _run(list_of_bytes, spec, tun, rows, sr, threads, feeders, device, errors, files_per_submit, stats):
    if errors not in ("raise", "return"):
        raise TuningError("errors must be 'raise' or 'return', got %r" % (errors,))
    target = check_sr(sr, TuningError)
    threads, feeders = _int("threads", threads, 0, 1 << 16), _int("feeders", feeders, 0, 1 << 16)
    device, files_per_submit = _int("device", device, 0, 1 << 16), _int("files_per_submit", files_per_submit, 1, 65535)
    lib = _load()
    n = len(list_of_bytes)
    nrows = np.zeros(max(n, 1), np.uint64)
    frames = np.zeros(max(n, 1), np.uint64)
    rates = np.zeros(max(n, 1), np.uint32)
    tunings = np.zeros(max(n, 1), np.float64)
    counts = np.zeros((max(n, 1), 2), np.uint64)
    nb = int(spec.n_fft) // 2 + 1

    def build(i, p):
        if not rows:
            return float(tunings[i]), int(rates[i])
        r = _corpus.copy_into(np.zeros((int(nrows[i]), 2 * nb), np.float32), p)
        return np.ascontiguousarray(r[:, :nb]), np.ascontiguousarray(r[:, nb:]), int(rates[i])

    res = _corpus.run(lib, lib.ogg_vorbis_tuning_corpus, list_of_bytes,
                      (threads, feeders, files_per_submit, device, target, C.byref(spec), C.byref(tun), 1 if rows else 0),
                      (nrows, frames, rates, tunings, counts), build, TuningError, errors, "tuning", stats)
    return res, counts[:n]


def get_tuning_batch(list_of_bytes, n_fft=2048, hop_length=None, win_length=None, center=True, power=1, fmin=150.0, fmax=4000.0,
                     threshold=0.1, resolution=0.01, bins_per_octave=12, sr=None, threads=0, feeders=0, device=0, errors="raise",
                     files_per_submit=64, stats=None, counts=None):
    """librosa.estimate_tuning of many Ogg Vorbis files in one corpus run: a list of (tuning, sr) tuples, tuning a float in
    [-0.5, 0.5) in fractions of a bin of bins_per_octave (0.0 for a file without a peak), sr the rate it was computed at.
    hop_length=None means n_fft // 4. sr, threads, feeders, errors and stats as for get_pcm_batch. counts (an optional list) receives
    per file (peaks, peaks at or above the median magnitude). A frame with an Inf or NaN sample contributes no peak."""
    spec, tun = framing_spec(n_fft, hop_length, win_length, center, power), tuning_spec(fmin, fmax, threshold, resolution, bins_per_octave)
    res, cnt = _run(list_of_bytes, spec, tun, False, sr, threads, feeders, device, errors, files_per_submit, stats)
    if counts is not None:
        counts[:] = [(int(a), int(b)) for a, b in cnt]
    return res


def get_piptrack_batch(list_of_bytes, n_fft=2048, hop_length=None, win_length=None, center=True, power=1, fmin=150.0, fmax=4000.0,
                       threshold=0.1, sr=None, threads=0, feeders=0, device=0, errors="raise", files_per_submit=64, stats=None):
    """librosa.piptrack's (pitches, magnitudes) of many files: a list of (pitches, mags, sr), both float32 (F, n_fft // 2 + 1), rows
    being frames (librosa's arrays transposed, as every row output here). A bin that is no peak holds 0 in both; a frame with an Inf or
    NaN sample is NaN throughout. The rest as get_tuning_batch."""
    spec, tun = framing_spec(n_fft, hop_length, win_length, center, power), tuning_spec(fmin, fmax, threshold)
    return _run(list_of_bytes, spec, tun, True, sr, threads, feeders, device, errors, files_per_submit, stats)[0]


def get_tuning_from_raw_bytes(raw_bytes, **kwargs):
    """One file's (tuning, sr), as get_tuning_batch."""
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return get_tuning_batch([raw_bytes], **kwargs)[0]


def get_piptrack_from_raw_bytes(raw_bytes, **kwargs):
    """One file's (pitches, mags, sr), as get_piptrack_batch."""
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return get_piptrack_batch([raw_bytes], **kwargs)[0]
