"""ctypes plumbing of the corpus front-ends (features.py, spectral.py, pcm.py, pitch.py, frame_descriptors.py, cqt.py, tuning.py, loudness.py): the corpus entry points of libparseoggvorbis_amd.so
and the per-file loop over the buffers they hand back (include/vorbis_synth_hip.h documents what they compute)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "host", "libparseoggvorbis_amd.so")

_lib = None


def load():
    """The host library with every corpus entry point's argtypes registered (loaded once)."""
    global _lib
    if _lib is not None:
        return _lib
    from . import binding
    binding.load()  # the HIP runtime (torch's, when torch is importable) before the host library
    if not os.path.exists(HOST_LIB_PATH):
        raise RuntimeError("host library missing: %s — run __graft_entry__.build() (there is no CPU fallback)" % HOST_LIB_PATH)
    lib = C.CDLL(HOST_LIB_PATH)
    vp, u32 = C.c_void_p, C.c_uint32
    head = [vp, vp, C.c_size_t, C.c_int, C.c_int, u32, C.c_int]  # datas, lens, num_files, threads, feeders, files_per_submit, device
    tail = [vp, vp, C.POINTER(C.c_char_p)]  # error_out_per_file, stats_out, error_out
    for name, args in (("ogg_vorbis_features_corpus", [C.POINTER(binding.FeatureSpec), vp, vp, vp]),
                       ("ogg_vorbis_spectral_corpus", [C.POINTER(binding.SpectralSpec), vp, vp, vp]),
                       ("ogg_vorbis_spectral_corpus_sr", [C.POINTER(binding.SpectralSpec), u32, vp, vp, vp]),
                       ("ogg_vorbis_spectral_corpus_post", [C.POINTER(binding.SpectralSpec), u32, C.POINTER(binding.SpectralPost), vp, vp, vp]),
                       ("ogg_vorbis_spectral_corpus_cond", [C.POINTER(binding.SpectralSpec), u32, C.POINTER(binding.SpectralPost),
                                                            C.POINTER(binding.PcmCond), vp, vp, vp]),
                       ("ogg_vorbis_pcm_corpus", [u32, C.c_int, vp, vp, vp, vp, vp]),
                       ("ogg_vorbis_spectral_corpus_trim", [C.POINTER(binding.SpectralSpec), u32, C.POINTER(binding.SpectralPost),
                                                            C.POINTER(binding.PcmCond), C.POINTER(binding.PcmTrim), vp, vp, vp, vp]),
                       ("ogg_vorbis_pcm_corpus_cond", [u32, C.c_int, C.POINTER(binding.PcmCond), vp, vp, vp, vp, vp]),
                       ("ogg_vorbis_pcm_corpus_trim", [u32, C.c_int, C.POINTER(binding.PcmCond), C.POINTER(binding.PcmTrim), vp, vp, vp, vp,
                                                       vp, vp]),
                       ("ogg_vorbis_pcm_corpus_split", [u32, C.c_int, C.POINTER(binding.PcmCond), C.POINTER(binding.PcmTrim), vp, vp, vp, vp,
                                                        vp, vp, vp]),
                       ("ogg_vorbis_spectral_corpus_split", [C.POINTER(binding.SpectralSpec), u32, C.POINTER(binding.SpectralPost),
                                                             C.POINTER(binding.PcmCond), C.POINTER(binding.PcmTrim), vp, vp, vp, vp, vp, vp]),
                       ("ogg_vorbis_spectral_corpus_pcen", [C.POINTER(binding.SpectralSpec), u32, C.POINTER(binding.SpectralPcen),
                                                            C.POINTER(binding.SpectralPost), C.POINTER(binding.PcmCond),
                                                            C.POINTER(binding.PcmTrim), C.c_int, vp, vp, vp, vp, vp, vp, vp]),
                       ("ogg_vorbis_intervals_corpus", [u32, C.POINTER(binding.PcmTrim), vp, vp, vp, vp, vp]),
                       ("ogg_vorbis_pitch_corpus", [u32, C.POINTER(binding.PitchSpec), vp, vp, vp, vp, vp]),
                       ("ogg_vorbis_pyin_corpus", [u32, C.POINTER(binding.PyinSpec), vp, vp, vp, vp, vp]),
                       ("ogg_vorbis_fdesc_corpus", [u32, C.POINTER(binding.FdescSpec), vp, vp, vp, vp, vp]),
                       ("ogg_vorbis_cqt_corpus", [u32, C.POINTER(binding.CqtSpec), vp, vp, vp, vp, vp]),
                       ("ogg_vorbis_cqt_corpus_est", [u32, C.POINTER(binding.CqtSpec), C.POINTER(binding.TuningSpec), vp, vp, vp, vp, vp, vp]),
                       ("ogg_vorbis_tuning_corpus", [u32, C.POINTER(binding.SpectralSpec), C.POINTER(binding.TuningSpec), C.c_int, vp, vp, vp,
                                                     vp, vp, vp, vp]),
                       ("ogg_vorbis_pcm_corpus_loud", [u32, C.c_int, C.POINTER(binding.PcmCond), C.POINTER(binding.PcmTrim), C.c_int,
                                                       C.POINTER(binding.LoudnessSpec), vp, vp, vp, vp, vp, vp, vp, vp, vp]),
                       ("ogg_vorbis_pcm_corpus_effects", [u32, C.c_int, C.POINTER(binding.PcmCond), C.POINTER(binding.PcmTrim), C.c_int,
                                                          C.POINTER(binding.PcmEffect), C.POINTER(binding.LoudnessSpec), vp, vp, vp, vp, vp, vp,
                                                          vp, vp, vp]),
                       ("ogg_vorbis_pcm_corpus_stretch", [u32, C.c_int, C.POINTER(binding.PcmCond), C.POINTER(binding.PcmTrim), C.c_int,
                                                          C.POINTER(binding.PcmEffect), C.POINTER(binding.PcmStretch), vp, vp,
                                                          C.POINTER(binding.LoudnessSpec), vp, vp, vp, vp, vp, vp, vp, vp, vp]),
                       ("ogg_vorbis_spectral_corpus_loud", [C.POINTER(binding.SpectralSpec), u32, C.POINTER(binding.SpectralPcen),
                                                            C.POINTER(binding.SpectralPost), C.POINTER(binding.PcmCond),
                                                            C.POINTER(binding.PcmTrim), C.c_int, C.POINTER(binding.LoudnessSpec), vp, vp, vp,
                                                            vp, vp, vp, vp, vp]),
                       ("ogg_vorbis_spectral_corpus_chroma", [C.POINTER(binding.SpectralSpec), C.POINTER(binding.SpectralChroma), u32,
                                                              C.POINTER(binding.SpectralPcen), C.POINTER(binding.SpectralPost),
                                                              C.POINTER(binding.PcmCond), C.POINTER(binding.PcmTrim), C.c_int,
                                                              C.POINTER(binding.LoudnessSpec), vp, vp, vp, vp, vp, vp, vp, vp]),
                       ("ogg_vorbis_spectral_corpus_chroma_est", [C.POINTER(binding.SpectralSpec), C.POINTER(binding.SpectralChroma), u32,
                                                                  C.POINTER(binding.SpectralPcen), C.POINTER(binding.SpectralPost),
                                                                  C.POINTER(binding.PcmCond), C.POINTER(binding.PcmTrim), C.c_int,
                                                                  C.POINTER(binding.LoudnessSpec), C.POINTER(binding.TuningSpec), vp, vp, vp,
                                                                  vp, vp, vp, vp, vp, vp]),
                       ("ogg_vorbis_spectral_corpus_hpss", [C.POINTER(binding.SpectralSpec), C.POINTER(binding.SpectralChroma), u32,
                                                            C.POINTER(binding.SpectralHpss), C.POINTER(binding.SpectralPcen),
                                                            C.POINTER(binding.SpectralPost), C.POINTER(binding.PcmCond),
                                                            C.POINTER(binding.PcmTrim), C.c_int, C.POINTER(binding.LoudnessSpec), vp, vp, vp, vp,
                                                            vp, vp, vp, vp]),
                       ("ogg_vorbis_rhythm_corpus", [C.POINTER(binding.SpectralSpec), C.POINTER(binding.SpectralChroma), u32,
                                                     C.POINTER(binding.SpectralHpss), C.POINTER(binding.SpectralPcen),
                                                     C.POINTER(binding.SpectralPost), C.POINTER(binding.RhythmSpec), C.POINTER(binding.PcmCond),
                                                     C.POINTER(binding.PcmTrim), C.c_int, C.POINTER(binding.LoudnessSpec), vp, vp, vp, vp,
                                                     vp, vp, vp, vp]),
                       ("ogg_vorbis_beats_corpus", [C.POINTER(binding.SpectralSpec), C.POINTER(binding.SpectralChroma), u32,
                                                    C.POINTER(binding.SpectralHpss), C.POINTER(binding.SpectralPcen),
                                                    C.POINTER(binding.SpectralPost), C.POINTER(binding.OnsetSpec), C.POINTER(binding.BeatSpec),
                                                    C.POINTER(binding.PcmCond), C.POINTER(binding.PcmTrim), C.c_int,
                                                    C.POINTER(binding.LoudnessSpec), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
                       ("ogg_vorbis_loudness_corpus", [u32, C.POINTER(binding.LoudnessSpec), C.c_int, vp, vp, vp, vp, vp, vp])):
        fn = getattr(lib, name)
        fn.argtypes = head + args + tail
        fn.restype = C.c_int
    lib.ogg_vorbis_features_free.argtypes = [vp]
    lib.ogg_vorbis_features_free.restype = None
    _lib = lib
    return lib


def check_errors(errors):
    if errors not in ("raise", "return"):
        raise ValueError("errors must be 'raise' or 'return'")


def run(lib, fn, list_of_bytes, args, arrays, build, error, errors, what, stats=None):
    """One corpus run of the C entry point fn over list_of_bytes: fn(datas, lens, n, *args, out, *arrays, ok, error_out_per_file,
    stats_out, error_out), arrays being the caller's per-file numpy outputs (or ctypes arrays). build(i, ptr) makes file i's entry from the buffer the
    library handed over (released here afterwards). A failed file raises error("file i: ...") (errors="raise") or is returned as
    one (errors="return"); a failed run raises error("<what> corpus run failed: ..."). stats (optional list) receives the run's 8
    corpus statistics."""
    n = len(list_of_bytes)
    if n == 0:
        return []
    bufs = [np.frombuffer(bytes(b), np.uint8) if len(b) else np.zeros(1, np.uint8) for b in list_of_bytes]
    datas = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[len(b) for b in list_of_bytes])
    out = (C.c_void_p * n)()
    ok = np.zeros(n, np.uint8)
    ferr = (C.c_char_p * n)()
    st = (C.c_double * 8)()
    err = C.c_char_p()
    if fn(datas, lens, n, *args, out, *[a.ctypes.data if isinstance(a, np.ndarray) else a for a in arrays], ok.ctypes.data, ferr, st,
          C.byref(err)) != 0:
        raise error("%s corpus run failed: %s" % (what, (err.value or b"").decode()))
    if stats is not None:
        stats[:] = list(st)
    res = []
    try:
        for i in range(n):
            if not ok[i]:
                e = error("file %d: %s" % (i, (ferr[i] or b"failed").decode(errors="replace")))
                if errors == "raise":
                    raise e
                res.append(e)
                continue
            res.append(build(i, out[i]))
    finally:
        for i in range(n):
            if out[i]:
                lib.ogg_vorbis_features_free(out[i])
    return res


class IntervalBuffers:
    """The per-file interval buffers of a split run: `ptrs` and `counts` go to the entry point (after its per-file output, or as
    it); take(i) is file i's (n, 2) int64 array; free() releases what the library handed over."""

    def __init__(self, lib, n):
        self.lib = lib
        self.ptrs = (C.c_void_p * max(n, 1))()
        self.counts = np.zeros(max(n, 1), np.uint64)

    def take(self, i):
        a = np.zeros((int(self.counts[i]), 2), np.uint32)
        return copy_into(a, self.ptrs[i]).astype(np.int64)

    def free(self):
        for i in range(len(self.ptrs)):
            if self.ptrs[i]:
                self.lib.ogg_vorbis_features_free(self.ptrs[i])
                self.ptrs[i] = None


def copy_into(a, ptr):
    """a, filled from the library's buffer at ptr (nothing to copy for an empty array)."""
    if a.size and ptr:
        C.memmove(a.ctypes.data, ptr, a.nbytes)
    return a
