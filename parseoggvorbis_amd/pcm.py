"""Decoded PCM from Ogg bytes, optionally resampled on the GPU: a list of (pcm, sr) like librosa.load. ctypes onto
libparseoggvorbis_amd.so (ogg_vorbis_pcm_corpus). Resampling is scipy.signal.resample_poly with its defaults (librosa's
res_type="polyphase", not its default soxr), computed on the device before the PCM is copied back; the arithmetic is written out
in include/vorbis_synth_hip.h ("resampling") and the float64 model in tests/resample_model.py is the contract.

Every argument is checked before the library is loaded."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "host", "libparseoggvorbis_amd.so")

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
    lib.ogg_vorbis_pcm_corpus.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_int, vp, vp, vp, vp,
                                          vp, vp, vp, C.POINTER(C.c_char_p)]
    lib.ogg_vorbis_pcm_corpus.restype = C.c_int
    lib.ogg_vorbis_features_free.argtypes = [vp]
    lib.ogg_vorbis_features_free.restype = None
    _lib = lib
    return lib


def get_pcm_batch(list_of_bytes, sr=None, dtype="float32", threads=0, feeders=0, device=0, errors="raise", files_per_submit=64,
                  stats=None):
    """PCM of many Ogg Vorbis files in one corpus run: a list of (pcm, sr) tuples. pcm is float32 (channels, frames), or int16
    (frames, channels) with ov_read's conversion; sr is the rate of the returned PCM. sr=None keeps each file's own rate (the
    PCM is bit for bit that of ogg_vorbis_decode_corpus); an integer resamples every file to it on the GPU. errors="raise": the
    first failed file raises PcmError naming it; errors="return": its entry is the PcmError. stats (optional list) receives
    the run's 8 corpus statistics."""
    if errors not in ("raise", "return"):
        raise ValueError("errors must be 'raise' or 'return'")
    target = check_sr(sr)
    name = _format(dtype)
    lib = _load()
    n = len(list_of_bytes)
    if n == 0:
        return []
    bufs = [np.frombuffer(bytes(b), np.uint8) if len(b) else np.zeros(1, np.uint8) for b in list_of_bytes]
    datas = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[len(b) for b in list_of_bytes])
    frames = np.zeros(n, np.uint64)
    chans = np.zeros(n, np.uint32)
    rates = np.zeros(n, np.uint32)
    ok = np.zeros(n, np.uint8)
    ferr = (C.c_char_p * n)()
    pcm = (C.c_void_p * n)()
    st = (C.c_double * 8)()
    err = C.c_char_p()
    rc = lib.ogg_vorbis_pcm_corpus(datas, lens, n, threads, feeders, files_per_submit, device, target, FORMATS[name], pcm,
                                   frames.ctypes.data, chans.ctypes.data, rates.ctypes.data, ok.ctypes.data, ferr, st, C.byref(err))
    if rc != 0:
        raise PcmError("pcm corpus run failed: %s" % (err.value or b"").decode())
    if stats is not None:
        stats[:] = list(st)
    res = []
    try:
        for i in range(n):
            if not ok[i]:
                e = PcmError("file %d: %s" % (i, (ferr[i] or b"failed").decode(errors="replace")))
                if errors == "raise":
                    raise e
                res.append(e)
                continue
            T, Cn = int(frames[i]), int(chans[i])
            a = np.zeros((Cn, T), np.float32) if name == "float32" else np.zeros((T, Cn), np.int16)
            if a.size and pcm[i]:
                C.memmove(a.ctypes.data, pcm[i], a.nbytes)
            res.append((a, int(rates[i])))
    finally:
        for i in range(n):
            if pcm[i]:
                lib.ogg_vorbis_features_free(pcm[i])
    return res


def get_pcm_from_raw_bytes(raw_bytes, sr=None, dtype="float32", **kwargs):
    """One file's (pcm, sr), as get_pcm_batch."""
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return get_pcm_batch([raw_bytes], sr, dtype, **kwargs)[0]
