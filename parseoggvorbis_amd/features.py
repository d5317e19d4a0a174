"""The reference's RETURNN feature matrices (returnn_import.py:74-115) computed on the GPU: Ogg bytes -> (time, output_dim) float32,
without synthesising PCM. ctypes onto libparseoggvorbis_amd.so (ogg_vorbis_features_corpus); the semantics, quirks included, are
documented in include/vorbis_synth_hip.h ("feature matrices").

Drop-in for RETURNN code: replace the reference's import of ParseOggVorbisLib with this module's; get_instance() and
get_features_from_raw_bytes(raw_bytes, output_dim, kind, **kwargs) keep the reference's names, kinds and keyword arguments.
Kind and keyword arguments are checked before the library is loaded."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "host", "libparseoggvorbis_amd.so")

KINDS = {"floor_final_ys": 1, "floor_final_ys_rendered": 2, "residue_ys": 3, "residue_ys_with_floor": 4}
NOT_PROVIDED = ("floor_final_ys_rendered_concat_residue",)
# keyword arguments of the reference's read_floor_ys / read_residue_ys (demo_live_extract.py:262-266, 418-419)
FLOOR_KWARGS = ("include_floor_number", "only_biggest_floor", "sorted_xs", "upscale_xs_factor", "xs_from_biggest_floor",
                "floor_always_positive", "verbose")
RESIDUE_KWARGS = ("scale", "clip_abs_max", "log1p_abs_space", "sorted_xs", "ignore_xs", "floor_base_factor")

OPT_INCLUDE_FLOOR_NUMBER, OPT_ONLY_BIGGEST_FLOOR, OPT_SORTED_XS, OPT_XS_FROM_BIGGEST_FLOOR = 1, 2, 4, 8
OPT_FLOOR_ALWAYS_POSITIVE, OPT_LOG1P_ABS_SPACE, OPT_IGNORE_XS, OPT_CLIP = 16, 32, 64, 128


class FeatureError(RuntimeError):
    pass


def feature_spec(output_dim, kind="floor_final_ys", **kwargs):
    """Checks kind and keyword arguments like the reference would and returns the C spec (binding.FeatureSpec)."""
    from .binding import FeatureSpec
    if kind in NOT_PROVIDED:
        raise FeatureError("get_features_from_raw_bytes: kind %r (the reference's scipy zoom order 3 over after_residue) is not "
                           "provided; supported kinds: %s" % (kind, ", ".join(sorted(KINDS))))
    if kind not in KINDS:
        raise FeatureError("get_features_from_raw_bytes: invalid kind %r; supported kinds: %s" % (kind, ", ".join(sorted(KINDS))))
    output_dim = int(output_dim)
    if output_dim < 1:
        raise FeatureError("output_dim must be >= 1, got %r" % output_dim)
    floor_kind = KINDS[kind] <= 2
    allowed = FLOOR_KWARGS if floor_kind else RESIDUE_KWARGS
    bad = sorted(set(kwargs) - set(allowed))
    if bad:  # the reference's reader raises TypeError for these
        raise TypeError("kind %r: unexpected keyword argument(s) %s (accepted: %s)" % (kind, ", ".join(bad), ", ".join(allowed)))
    opts, up, scale, clip, fbf = 0, 1.0, 1.0, 0.0, 1.0
    if kwargs.get("sorted_xs", False):
        opts |= OPT_SORTED_XS
    if floor_kind:
        include = kwargs.get("include_floor_number", None)
        if kwargs.get("only_biggest_floor", False):
            if include not in (None, False):
                raise AssertionError("only_biggest_floor excludes include_floor_number")  # the reference's assert
            opts |= OPT_ONLY_BIGGEST_FLOOR
            include = False
        if include is None or include:
            opts |= OPT_INCLUDE_FLOOR_NUMBER
        if kwargs.get("xs_from_biggest_floor", False):
            opts |= OPT_XS_FROM_BIGGEST_FLOOR
        if kwargs.get("floor_always_positive", False):
            opts |= OPT_FLOOR_ALWAYS_POSITIVE
        up = float(kwargs.get("upscale_xs_factor", 1))
        if not up > 0:
            raise FeatureError("upscale_xs_factor must be > 0, got %r" % up)
    else:
        if kwargs.get("log1p_abs_space", False):
            opts |= OPT_LOG1P_ABS_SPACE
        if kwargs.get("ignore_xs", False):
            opts |= OPT_IGNORE_XS
        scale = float(kwargs.get("scale", 1.0))
        c = kwargs.get("clip_abs_max", None)
        if c is not None and c > 0:
            opts |= OPT_CLIP
            clip = float(c)
        fbf = float(kwargs.get("floor_base_factor", 1))
    return FeatureSpec(KINDS[kind], output_dim, opts, 0, up, scale, clip, fbf, 0)


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
    lib.ogg_vorbis_features_corpus.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_int, C.POINTER(binding.FeatureSpec),
                                               vp, vp, vp, vp, vp, C.POINTER(C.c_char_p)]
    lib.ogg_vorbis_features_corpus.restype = C.c_int
    lib.ogg_vorbis_features_free.argtypes = [vp]
    lib.ogg_vorbis_features_free.restype = None
    _lib = lib
    return lib


def get_features_batch(list_of_bytes, output_dim, kind="floor_final_ys", threads=0, feeders=0, device=0, errors="raise",
                       files_per_submit=64, **kwargs):
    """Feature matrices of many Ogg Vorbis files in one corpus run. Returns a list of float32 arrays (rows, output_dim);
    errors="raise": the first failed file raises FeatureError naming it; errors="return": its entry is the FeatureError."""
    if errors not in ("raise", "return"):
        raise ValueError("errors must be 'raise' or 'return'")
    spec = feature_spec(output_dim, kind, **kwargs)
    lib = _load()
    n = len(list_of_bytes)
    if n == 0:
        return []
    bufs = [np.frombuffer(bytes(b), np.uint8) if len(b) else np.zeros(1, np.uint8) for b in list_of_bytes]
    datas = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[len(b) for b in list_of_bytes])
    # one pass: the library hands each file's rows over in a buffer of its own, copied here and released
    counts = np.zeros(n, np.uint64)
    ok = np.zeros(n, np.uint8)
    ferr = (C.c_char_p * n)()
    rows = (C.c_void_p * n)()
    err = C.c_char_p()
    rc = lib.ogg_vorbis_features_corpus(datas, lens, n, threads, feeders, files_per_submit, device, C.byref(spec), rows,
                                        counts.ctypes.data, ok.ctypes.data, ferr, None, C.byref(err))
    if rc != 0:
        raise FeatureError("features corpus run failed: %s" % (err.value or b"").decode())
    res = []
    try:
        for i in range(n):
            if not ok[i]:
                e = FeatureError("file %d: %s" % (i, (ferr[i] or b"failed").decode(errors="replace")))
                if errors == "raise":
                    raise e
                res.append(e)
                continue
            m = np.zeros((int(counts[i]), spec.output_dim), np.float32)
            if m.size:
                C.memmove(m.ctypes.data, rows[i], m.nbytes)
            res.append(m)
    finally:
        for i in range(n):
            if rows[i]:
                lib.ogg_vorbis_features_free(rows[i])
    return res


def get_features_from_raw_bytes(raw_bytes, output_dim, kind="floor_final_ys", **kwargs):
    """The reference's ParseOggVorbisLib.get_features_from_raw_bytes: shape (time, output_dim) float32."""
    return get_features_batch([raw_bytes], output_dim, kind, threads=1, feeders=1, **kwargs)[0]


class ParseOggVorbisLib:
    """Stand-in for the reference's class of the same name (returnn_import.py): one shared instance, same method."""
    instance = None

    @classmethod
    def get_instance(cls):
        if cls.instance is None:
            cls.instance = cls()
        return cls.instance

    def get_features_from_raw_bytes(self, raw_bytes, output_dim, kind="floor_final_ys", **kwargs):
        return get_features_from_raw_bytes(raw_bytes, output_dim, kind, **kwargs)
