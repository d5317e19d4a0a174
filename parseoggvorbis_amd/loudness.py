"""Integrated loudness (ITU-R BS.1770-4 / EBU R 128) from Ogg bytes, measured on the GPU: a list of (lufs, sr). ctypes onto
libparseoggvorbis_amd.so (ogg_vorbis_loudness_corpus). The measurement is the K-weighting filter, the 400 ms blocks at 75 % overlap
and the two gates of the standard on the decoded PCM, after the optional resampler and before anything is copied back: no PCM
crosses the bus. The arithmetic is written out in include/vorbis_synth_hip.h ("loudness") and the float64 model in
tests/loudness_model.py is the contract; for one and two channels it is the standard's measure (every channel has weight 1: the
surround weights and the LFE exclusion are not built), what pyloudnorm.Meter(sr).integrated_loudness computes, with which parity is
not claimed.

Every argument is checked before the library is loaded."""
import ctypes as C
import math

import numpy as np

from . import _corpus
from ._corpus import HOST_LIB_PATH  # noqa: F401
from .pcm import check_sr

LOUD_NORMALIZE = 1  # VSYN_LOUD_NORMALIZE
CHANNEL_MODES = {"sum": 0, "mono": 1}  # VSYN_LOUD_SUM, VSYN_LOUD_MONO
STATUS_SILENT = 3  # VSYN_LOUD_SILENT
MIN_RATE = 4000
TARGET_RANGE = (-70.0, 0.0)


class LoudnessError(RuntimeError):
    pass


def check_target(target, error=LoudnessError, name="target"):
    """A loudness target in LUFS: a finite number in [-70, 0]. Returns it as a float."""
    if isinstance(target, (bool, np.bool_)) or not isinstance(target, (int, float, np.integer, np.floating)):
        raise error("%s must be a number of LUFS, got %r" % (name, target))
    t = float(target)
    if not math.isfinite(t) or not TARGET_RANGE[0] <= t <= TARGET_RANGE[1]:
        raise error("%s must be finite and in [%g, %g] LUFS, got %r" % (name, TARGET_RANGE[0], TARGET_RANGE[1], target))
    return t


def loudness_spec(channels="sum", target=None, error=LoudnessError):
    """Checks the arguments (include/vorbis_synth_hip.h, "loudness", step 6) and returns the C spec (binding.LoudnessSpec): channels
    "sum" (every channel plane, unit weights) or "mono" (the mono downmix of get_pcm_batch(mono=True)); target None (measure only)
    or a number of LUFS in [-70, 0]."""
    from .binding import LoudnessSpec
    if not isinstance(channels, str) or channels not in CHANNEL_MODES:
        raise error("channels must be 'sum' or 'mono', got %r" % (channels,))
    if target is None:
        return LoudnessSpec(0, CHANNEL_MODES[channels], 0.0)
    return LoudnessSpec(LOUD_NORMALIZE, CHANNEL_MODES[channels], check_target(target, error))


def lufs_of(z):
    """-0.691 + 10 log10(z) for a mean square z (a float or an array): -inf for 0."""
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(np.asarray(z, np.float64))


_load = _corpus.load


def get_loudness_batch(list_of_bytes, sr=None, channels="sum", blocks=False, threads=0, feeders=0, device=0, errors="raise",
                       files_per_submit=64, stats=None):
    """The integrated loudness of many Ogg Vorbis files in one corpus run: a list of (lufs, sr) tuples, lufs a float in LUFS, sr the
    rate it was measured at (sr, or the file's own for sr=None). channels="sum" measures the file's channel planes with unit
    weights (the standard's measure for mono and stereo), "mono" their downmix, the signal get_pcm_batch(mono=True) returns. With
    blocks=True each entry is (lufs, sr, block_lufs): float64 (n_blocks,), the loudness of every 400 ms block in front of the gates.
    sr, errors and stats as for get_pcm_batch. A silent file (no block above -70 LUFS) gives -inf and is not an error; a file
    shorter than 400 ms, with an Inf or NaN sample or with a rate below 4000 Hz fails alone: errors="raise" raises LoudnessError
    naming the first such file, errors="return" puts the LoudnessError in its slot."""
    _corpus.check_errors(errors)
    target = check_sr(sr, LoudnessError)
    if target and target < MIN_RATE:
        raise LoudnessError("sr must be at least %d Hz for a loudness measurement, got %r" % (MIN_RATE, sr))
    if not isinstance(blocks, (bool, np.bool_)):
        raise LoudnessError("blocks must be a bool, got %r" % (blocks,))
    spec = loudness_spec(channels)
    from .binding import LOUDNESS_RECORD_DTYPE
    lib = _load()
    n = len(list_of_bytes)
    counts = np.zeros(max(n, 1), np.uint64)
    records = np.zeros(max(n, 1), LOUDNESS_RECORD_DTYPE)
    frames = np.zeros(max(n, 1), np.uint64)
    rates = np.zeros(max(n, 1), np.uint32)

    def build(i, p):
        rec = records[i]
        loud = -math.inf if rec["status"] == STATUS_SILENT else float(lufs_of(rec["zbar"]))
        if not blocks:
            return loud, int(rates[i])
        return loud, int(rates[i]), lufs_of(_corpus.copy_into(np.zeros(int(counts[i]), np.float64), p))

    return _corpus.run(lib, lib.ogg_vorbis_loudness_corpus, list_of_bytes,
                       (threads, feeders, files_per_submit, device, target, C.byref(spec), 1 if blocks else 0),
                       (counts, records, frames, rates), build, LoudnessError, errors, "loudness", stats)


def get_loudness_from_raw_bytes(raw_bytes, **kwargs):
    """One file's (lufs, sr) or (lufs, sr, block_lufs), as get_loudness_batch."""
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return get_loudness_batch([raw_bytes], **kwargs)[0]
