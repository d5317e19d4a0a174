"""The reference's RETURNN feature matrices (returnn_import.py:74-115) computed on the GPU: Ogg bytes -> (time, output_dim) float32,
without synthesising PCM. ctypes onto libparseoggvorbis_amd.so (ogg_vorbis_features_corpus); the semantics, quirks included, are
documented in include/vorbis_synth_hip.h ("feature matrices").

Drop-in for RETURNN code: replace the reference's import of ParseOggVorbisLib with this module's; get_instance() and
get_features_from_raw_bytes(raw_bytes, output_dim, kind, **kwargs) keep the reference's names, kinds and keyword arguments.
Kind and keyword arguments are checked before the library is loaded."""
import ctypes as C

import numpy as np

from . import _corpus
from ._corpus import HOST_LIB_PATH  # noqa: F401

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


_load = _corpus.load


def get_features_batch(list_of_bytes, output_dim, kind="floor_final_ys", threads=0, feeders=0, device=0, errors="raise",
                       files_per_submit=64, **kwargs):
    """Feature matrices of many Ogg Vorbis files in one corpus run. Returns a list of float32 arrays (rows, output_dim);
    errors="raise": the first failed file raises FeatureError naming it; errors="return": its entry is the FeatureError."""
    _corpus.check_errors(errors)
    spec = feature_spec(output_dim, kind, **kwargs)
    lib = _load()
    counts = np.zeros(len(list_of_bytes), np.uint64)
    # one pass: the library hands each file's rows over in a buffer of its own, copied here and released
    return _corpus.run(lib, lib.ogg_vorbis_features_corpus, list_of_bytes, (threads, feeders, files_per_submit, device, C.byref(spec)),
                       (counts,), lambda i, p: _corpus.copy_into(np.zeros((int(counts[i]), spec.output_dim), np.float32), p),
                       FeatureError, errors, "features")


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
