"""Decoded PCM from Ogg bytes, optionally resampled on the GPU: a list of (pcm, sr) like librosa.load. ctypes onto
libparseoggvorbis_amd.so (ogg_vorbis_pcm_corpus). Resampling is scipy.signal.resample_poly with its defaults (librosa's
res_type="polyphase", not its default soxr), computed on the device before the PCM is copied back; the arithmetic is written out
in include/vorbis_synth_hip.h ("resampling") and the float64 model in tests/resample_model.py is the contract.

Every argument is checked before the library is loaded."""
import numpy as np

from . import _corpus
from ._corpus import HOST_LIB_PATH  # noqa: F401

FORMATS = {"float32": 2, "int16": 1}  # VSYN_PCM_F32, VSYN_PCM_S16
MAX_RATE = 0xFFFFFFFF


class PcmError(RuntimeError):
    pass


def check_sr(sr, error=PcmError):
    """None (each file's own rate) or a positive integer rate in Hz; returns the C target rate (0 = native)."""
    if sr is None:
        return 0
    if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)):
        raise error("sr must be None or a positive integer (Hz), got %r" % (sr,))
    if not 1 <= int(sr) <= MAX_RATE:
        raise error("sr must be in [1, %d] Hz, got %d" % (MAX_RATE, int(sr)))
    return int(sr)


def _format(dtype):
    name = dtype if isinstance(dtype, str) else getattr(dtype, "__name__", None)
    if isinstance(dtype, np.dtype):
        name = dtype.name
    if name not in FORMATS:
        raise PcmError("dtype must be 'float32' or 'int16', got %r" % (dtype,))
    return name


_load = _corpus.load


def get_pcm_batch(list_of_bytes, sr=None, dtype="float32", threads=0, feeders=0, device=0, errors="raise", files_per_submit=64,
                  stats=None):
    """PCM of many Ogg Vorbis files in one corpus run: a list of (pcm, sr) tuples. pcm is float32 (channels, frames), or int16
    (frames, channels) with ov_read's conversion; sr is the rate of the returned PCM. sr=None keeps each file's own rate (the
    PCM is bit for bit that of ogg_vorbis_decode_corpus); an integer resamples every file to it on the GPU. errors="raise": the
    first failed file raises PcmError naming it; errors="return": its entry is the PcmError. stats (optional list) receives
    the run's 8 corpus statistics."""
    _corpus.check_errors(errors)
    target = check_sr(sr)
    name = _format(dtype)
    lib = _load()
    n = len(list_of_bytes)
    frames = np.zeros(n, np.uint64)
    chans = np.zeros(n, np.uint32)
    rates = np.zeros(n, np.uint32)

    def build(i, p):
        T, Cn = int(frames[i]), int(chans[i])
        a = np.zeros((Cn, T), np.float32) if name == "float32" else np.zeros((T, Cn), np.int16)
        return _corpus.copy_into(a, p), int(rates[i])

    return _corpus.run(lib, lib.ogg_vorbis_pcm_corpus, list_of_bytes, (threads, feeders, files_per_submit, device, target, FORMATS[name]),
                       (frames, chans, rates), build, PcmError, errors, "pcm", stats)


def get_pcm_from_raw_bytes(raw_bytes, sr=None, dtype="float32", **kwargs):
    """One file's (pcm, sr), as get_pcm_batch."""
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return get_pcm_batch([raw_bytes], sr, dtype, **kwargs)[0]
