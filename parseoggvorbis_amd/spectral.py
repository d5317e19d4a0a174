"""Spectral front-end features computed on the GPU from Ogg bytes: mel power, log-mel, dB-mel and MFCC matrices
(frames, dim) float32, from the decoded PCM while it is still on the device (no PCM crosses the bus). ctypes onto
libparseoggvorbis_amd.so (ogg_vorbis_spectral_corpus); the semantics are documented in include/vorbis_synth_hip.h ("spectral
features"). They follow librosa's documented defaults (librosa >= 0.10); parity with librosa itself has not been verified, the
float64 model in tests/spectral_model.py is the contract the device is tested against.

Every argument is checked before the library is loaded. 25 ms / 10 ms at 44.1 kHz: n_fft=1102, hop_length=441. sr=None computes
each file's matrix at its own rate; an integer sr resamples every file's PCM to it on the device first (parseoggvorbis_amd/pcm.py,
scipy.signal.resample_poly's arithmetic), so that one mel table serves the whole batch."""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "host", "libparseoggvorbis_amd.so")

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


_lib = None


def _load():
    global _lib
    if _lib is not None:
        return _lib
    from . import binding
    binding.load()  # the HIP runtime (torch's, when torch is importable) before the host library
    if not os.path.exists(HOST_LIB_PATH):
        raise RuntimeError("host library missing: %s — run __graft_entry__.build() (there is no CPU fallback)" % HOST_LIB_PATH)
    lib = C.CDLL(HOST_LIB_PATH)
    vp = C.c_void_p
    lib.ogg_vorbis_spectral_corpus.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_int, C.POINTER(binding.SpectralSpec),
                                               vp, vp, vp, vp, vp, C.POINTER(C.c_char_p)]
    lib.ogg_vorbis_spectral_corpus.restype = C.c_int
    lib.ogg_vorbis_spectral_corpus_sr.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_int,
                                                  C.POINTER(binding.SpectralSpec), C.c_uint32, vp, vp, vp, vp, vp, C.POINTER(C.c_char_p)]
    lib.ogg_vorbis_spectral_corpus_sr.restype = C.c_int
    lib.ogg_vorbis_features_free.argtypes = [vp]
    lib.ogg_vorbis_features_free.restype = None
    _lib = lib
    return lib


def get_spectral_batch(list_of_bytes, kind="log_mel", n_fft=2048, hop_length=512, win_length=None, n_mels=128, fmin=0.0, fmax=None,
                       htk=False, norm="slaney", center=True, power=2.0, log_floor=1e-3, amin=1e-10, top_db=80.0, n_mfcc=20,
                       threads=0, feeders=0, device=0, errors="raise", files_per_submit=64, stats=None, sr=None):
    """Spectral matrices of many Ogg Vorbis files in one corpus run: a list of float32 arrays (frames, dim), dim = n_mfcc for
    "mfcc", n_mels otherwise. errors="raise": the first failed file raises SpectralError naming it; errors="return": its entry
    is the SpectralError. stats (optional list) receives the run's 8 corpus statistics. sr=None: each file at its own rate;
    an integer: every file resampled to sr on the device, and the mel table and the fmin / fmax check use sr."""
    if errors not in ("raise", "return"):
        raise ValueError("errors must be 'raise' or 'return'")
    from .pcm import check_sr
    target = check_sr(sr, SpectralError)
    spec = spectral_spec(kind, n_fft, hop_length, win_length, n_mels, fmin, fmax, htk, norm, center, power, log_floor, amin, top_db,
                         n_mfcc)
    lib = _load()
    n = len(list_of_bytes)
    if n == 0:
        return []
    dim = spec_dim(spec)
    bufs = [np.frombuffer(bytes(b), np.uint8) if len(b) else np.zeros(1, np.uint8) for b in list_of_bytes]
    datas = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[len(b) for b in list_of_bytes])
    counts = np.zeros(n, np.uint64)
    ok = np.zeros(n, np.uint8)
    ferr = (C.c_char_p * n)()
    rows = (C.c_void_p * n)()
    st = (C.c_double * 8)()
    err = C.c_char_p()
    if target:
        rc = lib.ogg_vorbis_spectral_corpus_sr(datas, lens, n, threads, feeders, files_per_submit, device, C.byref(spec), target, rows,
                                               counts.ctypes.data, ok.ctypes.data, ferr, st, C.byref(err))
    else:
        rc = lib.ogg_vorbis_spectral_corpus(datas, lens, n, threads, feeders, files_per_submit, device, C.byref(spec), rows,
                                            counts.ctypes.data, ok.ctypes.data, ferr, st, C.byref(err))
    if rc != 0:
        raise SpectralError("spectral corpus run failed: %s" % (err.value or b"").decode())
    if stats is not None:
        stats[:] = list(st)
    res = []
    try:
        for i in range(n):
            if not ok[i]:
                e = SpectralError("file %d: %s" % (i, (ferr[i] or b"failed").decode(errors="replace")))
                if errors == "raise":
                    raise e
                res.append(e)
                continue
            m = np.zeros((int(counts[i]), dim), np.float32)
            if m.size:
                C.memmove(m.ctypes.data, rows[i], m.nbytes)
            res.append(m)
    finally:
        for i in range(n):
            if rows[i]:
                lib.ogg_vorbis_features_free(rows[i])
    return res


def get_spectral_from_raw_bytes(raw_bytes, kind="log_mel", **kwargs):
    """One file's spectral matrix, shape (frames, dim) float32."""
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return get_spectral_batch([raw_bytes], kind, **kwargs)[0]
