"""Spectral front-end features computed on the GPU from Ogg bytes: mel power, log-mel, dB-mel and MFCC matrices
(frames, dim) float32, from the decoded PCM while it is still on the device (no PCM crosses the bus). ctypes onto
libparseoggvorbis_amd.so (ogg_vorbis_spectral_corpus_sr); the semantics are documented in include/vorbis_synth_hip.h ("spectral
features"). They follow librosa's documented defaults (librosa >= 0.10); parity with librosa itself has not been verified, the
float64 model in tests/spectral_model.py is the contract the device is tested against.

Every argument is checked before the library is loaded. 25 ms / 10 ms at 44.1 kHz: n_fft=1102, hop_length=441. sr=None computes
each file's matrix at its own rate; an integer sr resamples every file's PCM to it on the device first (parseoggvorbis_amd/pcm.py,
scipy.signal.resample_poly's arithmetic), so that one mel table serves the whole batch."""
import ctypes as C
import math

import numpy as np

from . import _corpus
from ._corpus import HOST_LIB_PATH  # noqa: F401

KINDS = {"mel_power": 1, "log_mel": 2, "mel_db": 3, "mfcc": 4}
OPT_CENTER, OPT_HTK, OPT_NO_NORM = 1, 2, 4
MAX_N_FFT, MAX_N_MELS = 8192, 256


class SpectralError(RuntimeError):
    pass


def _int(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise SpectralError("%s must be an integer, got %r" % (name, v))
    return int(v)


def spectral_spec(kind="log_mel", n_fft=2048, hop_length=512, win_length=None, n_mels=128, fmin=0.0, fmax=None, htk=False,
                  norm="slaney", center=True, power=2.0, log_floor=1e-3, amin=1e-10, top_db=80.0, n_mfcc=20):
    """Checks the arguments (include/vorbis_synth_hip.h, "spectral features", step 7; fmax against each file's rate happens per
    file) and returns the C spec (binding.SpectralSpec)."""
    from .binding import SpectralSpec
    if kind not in KINDS:
        raise SpectralError("invalid spectral kind %r; supported kinds: %s" % (kind, ", ".join(sorted(KINDS))))
    n_fft = _int("n_fft", n_fft)
    hop_length = _int("hop_length", hop_length)
    win_length = n_fft if win_length is None else _int("win_length", win_length)
    n_mels = _int("n_mels", n_mels)
    n_mfcc = _int("n_mfcc", n_mfcc)
    if not 16 <= n_fft <= MAX_N_FFT:
        raise SpectralError("n_fft must be in [16, %d], got %d" % (MAX_N_FFT, n_fft))
    if hop_length < 1:
        raise SpectralError("hop_length must be >= 1, got %d" % hop_length)
    if not 1 <= win_length <= n_fft:
        raise SpectralError("win_length must be in [1, n_fft=%d], got %d" % (n_fft, win_length))
    if not 1 <= n_mels <= MAX_N_MELS:
        raise SpectralError("n_mels must be in [1, %d], got %d" % (MAX_N_MELS, n_mels))
    if kind == "mfcc" and not 1 <= n_mfcc <= n_mels:
        raise SpectralError("n_mfcc must be in [1, n_mels=%d], got %d" % (n_mels, n_mfcc))
    if power not in (1, 2, 1.0, 2.0) or isinstance(power, bool):
        raise SpectralError("power must be 1 or 2, got %r" % (power,))
    if norm not in ("slaney", None):
        raise SpectralError("norm must be 'slaney' or None, got %r" % (norm,))
    fmin = float(fmin)
    fmax = 0.0 if fmax is None else float(fmax)
    if not (math.isfinite(fmin) and fmin >= 0.0):
        raise SpectralError("fmin must be >= 0, got %r" % fmin)
    if fmax != 0.0 and not (math.isfinite(fmax) and fmax > fmin):
        raise SpectralError("fmax must be above fmin=%g, got %r" % (fmin, fmax))
    log_floor, amin = float(log_floor), float(amin)
    top_db = 0.0 if top_db is None else float(top_db)
    if kind == "log_mel" and not log_floor > 0:
        raise SpectralError("log_floor must be > 0, got %r" % log_floor)
    if kind in ("mel_db", "mfcc") and not amin > 0:
        raise SpectralError("amin must be > 0, got %r" % amin)
    if kind in ("mel_db", "mfcc") and not top_db >= 0:
        raise SpectralError("top_db must be >= 0 (or None), got %r" % top_db)
    opts = (OPT_CENTER if center else 0) | (OPT_HTK if htk else 0) | (OPT_NO_NORM if norm is None else 0)
    return SpectralSpec(KINDS[kind], opts, n_fft, hop_length, win_length, n_mels, n_mfcc if kind == "mfcc" else 0, int(power),
                        fmin, fmax, log_floor, amin, top_db)


def spec_dim(spec):
    return spec.n_mfcc if spec.kind == KINDS["mfcc"] else spec.n_mels


_load = _corpus.load


def get_spectral_batch(list_of_bytes, kind="log_mel", n_fft=2048, hop_length=512, win_length=None, n_mels=128, fmin=0.0, fmax=None,
                       htk=False, norm="slaney", center=True, power=2.0, log_floor=1e-3, amin=1e-10, top_db=80.0, n_mfcc=20,
                       threads=0, feeders=0, device=0, errors="raise", files_per_submit=64, stats=None, sr=None):
    """Spectral matrices of many Ogg Vorbis files in one corpus run: a list of float32 arrays (frames, dim), dim = n_mfcc for
    "mfcc", n_mels otherwise. errors="raise": the first failed file raises SpectralError naming it; errors="return": its entry
    is the SpectralError. stats (optional list) receives the run's 8 corpus statistics. sr=None: each file at its own rate;
    an integer: every file resampled to sr on the device, and the mel table and the fmin / fmax check use sr."""
    _corpus.check_errors(errors)
    from .pcm import check_sr
    target = check_sr(sr, SpectralError)
    spec = spectral_spec(kind, n_fft, hop_length, win_length, n_mels, fmin, fmax, htk, norm, center, power, log_floor, amin, top_db,
                         n_mfcc)
    lib = _load()
    dim = spec_dim(spec)
    counts = np.zeros(len(list_of_bytes), np.uint64)
    return _corpus.run(lib, lib.ogg_vorbis_spectral_corpus_sr, list_of_bytes,
                       (threads, feeders, files_per_submit, device, C.byref(spec), target), (counts,),
                       lambda i, p: _corpus.copy_into(np.zeros((int(counts[i]), dim), np.float32), p), SpectralError, errors, "spectral",
                       stats)


def get_spectral_from_raw_bytes(raw_bytes, kind="log_mel", **kwargs):
    """One file's spectral matrix, shape (frames, dim) float32."""
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return get_spectral_batch([raw_bytes], kind, **kwargs)[0]
