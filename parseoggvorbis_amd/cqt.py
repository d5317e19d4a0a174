"""Constant-Q / variable-Q rows and the chroma_cqt (or tonnetz) rows folded from them, from Ogg bytes, computed on the GPU: a list of
(rows, sr). ctypes onto libparseoggvorbis_amd.so (ogg_vorbis_cqt_corpus). The transform is the direct time-domain sum that
librosa.cqt / librosa.vqt approximate (no sparsified FFT basis, no recursive decimation), on the mono signal
y = get_pcm_batch(mono=True, sr=sr), after the optional resampler and before anything is copied back: no PCM crosses the bus. The
arithmetic is written out in include/vorbis_synth_hip.h ("constant-Q") and the float64 model in tests/cqt_model.py is the contract;
parity with librosa itself is not claimed. Row t is centred on sample t * hop_length, as row t of get_spectral_batch(center=True) with
an even n_fft and frame t of get_f0_batch / get_frame_descriptors_batch (center=True) are.

Every argument is checked before the library is loaded."""
import ctypes as C
import math

import numpy as np

from . import _corpus
from ._corpus import HOST_LIB_PATH  # noqa: F401
from .pcm import U32_MAX, check_sr

C1 = 32.70319566257483  # librosa.note_to_hz("C1"), the default fmin
CQT_SCALE, CQT_BASE_C = 1, 2  # VSYN_CQT_SCALE, VSYN_CQT_BASE_C
OUTPUTS = {"magnitude": 1, "complex": 2, "chroma": 3, "tonnetz": 4}  # VSYN_CQT_MAG ..
CHROMA_NORMS = {None: 0, 1: 1, 2: 2, np.inf: 3}  # VSYN_CHROMA_NORM_*
MAX_BINS = 256


class CqtError(RuntimeError):
    pass


def _real(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise CqtError("%s must be a number, got %r" % (name, v))
    if not math.isfinite(float(v)):
        raise CqtError("%s must be finite, got %r" % (name, v))
    return float(v)


def _int(name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise CqtError("%s must be an integer, got %r" % (name, v))
    if not lo <= int(v) <= hi:
        raise CqtError("%s must be in [%d, %d], got %d" % (name, lo, hi, int(v)))
    return int(v)


def _bool(name, v):
    if not isinstance(v, (bool, np.bool_)):
        raise CqtError("%s must be a bool, got %r" % (name, v))
    return bool(v)


def _choice(name, v, table):
    if isinstance(v, (bool, np.bool_)):
        raise CqtError("%s must be one of %r, got %r" % (name, list(table), v))
    try:
        return table[v]
    except (KeyError, TypeError):
        raise CqtError("%s must be one of %r, got %r" % (name, list(table), v)) from None


def cqt_spec(hop_length=512, fmin=None, n_bins=84, bins_per_octave=12, tuning=0.0, filter_scale=1.0, gamma=0.0, norm=1, scale=True,
             output="magnitude", power=1, n_chroma=12, chroma_norm=np.inf, base_c=True):
    """Checks the arguments (include/vorbis_synth_hip.h, "constant-Q", step 11) and returns the C spec (binding.CqtSpec): n_bins and
    bins_per_octave integers in [1, 256]; hop_length an integer >= 1; fmin None (C1) or finite and > 0; filter_scale finite and > 0;
    gamma finite and >= 0; tuning finite; norm 1, 2 or None; scale a bool; output one of OUTPUTS; power 1 or 2; for the chroma
    outputs n_chroma an integer in [1, 256] that divides bins_per_octave, chroma_norm inf, 1, 2 or None, base_c a bool."""
    from .binding import CqtSpec
    hop = _int("hop_length", hop_length, 1, U32_MAX)
    nb = _int("n_bins", n_bins, 1, MAX_BINS)
    bpo = _int("bins_per_octave", bins_per_octave, 1, 256)
    f = C1 if fmin is None else _real("fmin", fmin)
    if not f > 0.0:
        raise CqtError("fmin must be > 0, got %r" % (fmin,))
    if tuning is None:
        raise CqtError("tuning must be a number, got None (librosa's tuning=None is tuning=\"estimate\" in the batch functions)")
    fs, gm, tu = _real("filter_scale", filter_scale), _real("gamma", gamma), _real("tuning", tuning)
    if not fs > 0.0:
        raise CqtError("filter_scale must be > 0, got %r" % (filter_scale,))
    if not gm >= 0.0:
        raise CqtError("gamma must be >= 0, got %r" % (gamma,))
    nrm = _choice("norm", norm, {None: 0, 1: 1, 2: 2})
    opts = CQT_SCALE if _bool("scale", scale) else 0
    out = _choice("output", output, OUTPUTS)
    pw = _choice("power", power, {1: 1, 2: 2})
    nc, cn = 0, 0
    if out >= OUTPUTS["chroma"]:
        nc = _int("n_chroma", n_chroma, 1, 256)
        if bpo % nc:
            raise CqtError("bins_per_octave %d is no multiple of n_chroma %d" % (bpo, nc))
        cn = _choice("chroma_norm", chroma_norm, CHROMA_NORMS)
        opts |= CQT_BASE_C if _bool("base_c", base_c) else 0
    return CqtSpec(nb, bpo, hop, opts, out, pw, nrm, nc, cn, 0, f, tu, fs, gm)


_load = _corpus.load


def _estimate(tuning, bins_per_octave, resolution, fmin, fmax, threshold):
    """(the number cqt_spec gets, the estimator's C spec or None): tuning="estimate" is librosa's tuning=None, each file's own estimate
    first (parseoggvorbis_amd/tuning.py); None itself and every other string stay refused by cqt_spec."""
    if not (isinstance(tuning, str) and tuning == "estimate"):
        return tuning, None
    from .tuning import TuningError, tuning_spec
    try:
        return 0.0, tuning_spec(fmin, fmax, threshold, resolution, _int("bins_per_octave", bins_per_octave, 1, 256))
    except TuningError as e:
        raise CqtError("tuning='estimate': tuning_%s" % e) from None


def _run(list_of_bytes, spec, sr, threads, feeders, device, errors, files_per_submit, stats, est=None):
    if errors not in ("raise", "return"):
        raise CqtError("errors must be 'raise' or 'return', got %r" % (errors,))
    target = check_sr(sr, CqtError)
    threads, feeders = _int("threads", threads, 0, 1 << 16), _int("feeders", feeders, 0, 1 << 16)
    device, files_per_submit = _int("device", device, 0, 1 << 16), _int("files_per_submit", files_per_submit, 1, 65535)
    lib = _load()
    n = len(list_of_bytes)
    counts = np.zeros(max(n, 1), np.uint64)
    frames = np.zeros(max(n, 1), np.uint64)
    rates = np.zeros(max(n, 1), np.uint32)
    nb = int(spec.n_bins)
    dim = {1: nb, 2: 2 * nb, 3: int(spec.n_chroma), 4: 6}[int(spec.output)]

    tunings = np.zeros(max(n, 1), np.float64)

    def build(i, p):
        rows = _corpus.copy_into(np.zeros((int(counts[i]), dim), np.float32), p)
        if spec.output == OUTPUTS["complex"]:
            rows = rows.view(np.complex64)
        return (rows, int(rates[i])) if est is None else (rows, int(rates[i]), float(tunings[i]))

    if est is not None:
        return _corpus.run(lib, lib.ogg_vorbis_cqt_corpus_est, list_of_bytes,
                           (threads, feeders, files_per_submit, device, target, C.byref(spec), C.byref(est)), (counts, frames, rates, tunings), build,
                           CqtError, errors, "constant-Q", stats)
    return _corpus.run(lib, lib.ogg_vorbis_cqt_corpus, list_of_bytes, (threads, feeders, files_per_submit, device, target, C.byref(spec)),
                       (counts, frames, rates), build, CqtError, errors, "constant-Q", stats)


def get_cqt_batch(list_of_bytes, hop_length=512, fmin=None, n_bins=84, bins_per_octave=12, tuning=0.0, filter_scale=1.0, gamma=0.0, norm=1,
                  scale=True, output="magnitude", power=1, sr=None, threads=0, feeders=0, device=0, errors="raise", files_per_submit=64,
                  stats=None, tuning_resolution=0.01, tuning_fmin=150.0, tuning_fmax=4000.0, tuning_threshold=0.1):
    """The constant-Q (gamma = 0) or variable-Q (gamma > 0) rows of many Ogg Vorbis files in one corpus run: a list of (rows, sr)
    tuples. rows is float32 (F, n_bins), |C|^power, for output="magnitude" and complex64 (F, n_bins) for output="complex",
    F = 1 + T // hop_length; sr is the rate they were computed at. fmin=None means C1. sr, threads, feeders, errors and stats as for
    get_pcm_batch. A file with an Inf or NaN sample, and a file at whose rate the top bin's pass band leaves the Nyquist band, fails
    alone: errors="raise" raises CqtError naming the first such file and which of the two it was, errors="return" puts the CqtError in
    its slot. tuning="estimate" (librosa's tuning=None; None itself stays refused): each file's tuning is estimated first on the device
    from a magnitude STFT (n_fft 2048, hop 512) of the signal the transform sees, with tuning_fmin, tuning_fmax, tuning_threshold,
    tuning_resolution and the transform's bins_per_octave; the entries are then (rows, sr, tuning), the rows those of the same call with
    that number, bit for bit."""
    if output not in ("magnitude", "complex"):
        raise CqtError("output must be 'magnitude' or 'complex', got %r" % (output,))
    tuning, est = _estimate(tuning, bins_per_octave, tuning_resolution, tuning_fmin, tuning_fmax, tuning_threshold)
    spec = cqt_spec(hop_length, fmin, n_bins, bins_per_octave, tuning, filter_scale, gamma, norm, scale, output, power)
    return _run(list_of_bytes, spec, sr, threads, feeders, device, errors, files_per_submit, stats, est)


def get_chroma_cqt_batch(list_of_bytes, hop_length=512, fmin=None, n_chroma=12, n_octaves=7, bins_per_octave=36, tuning=0.0, filter_scale=1.0,
                         gamma=0.0, norm=1, scale=True, chroma_norm=np.inf, base_c=True, tonnetz=False, sr=None, threads=0, feeders=0,
                         device=0, errors="raise", files_per_submit=64, stats=None, tuning_resolution=0.01, tuning_fmin=150.0,
                         tuning_fmax=4000.0, tuning_threshold=0.1):
    """librosa.feature.chroma_cqt's rows (threshold=None, cqt_mode="full", window=None) of many files: a list of (rows, sr), rows
    float32 (F, n_chroma), or with tonnetz=True the (F, 6) tonnetz rows computed from them. The transform has
    n_bins = n_octaves * bins_per_octave bins (at most 256). The rest as get_cqt_batch, tuning="estimate" included."""
    no = _int("n_octaves", n_octaves, 1, MAX_BINS)
    bpo = _int("bins_per_octave", bins_per_octave, 1, 256)
    if no * bpo > MAX_BINS:
        raise CqtError("n_octaves * bins_per_octave = %d exceeds %d bins" % (no * bpo, MAX_BINS))
    tuning, est = _estimate(tuning, bpo, tuning_resolution, tuning_fmin, tuning_fmax, tuning_threshold)
    spec = cqt_spec(hop_length, fmin, no * bpo, bpo, tuning, filter_scale, gamma, norm, scale, "tonnetz" if _bool("tonnetz", tonnetz) else "chroma",
                    1, n_chroma, chroma_norm, base_c)
    return _run(list_of_bytes, spec, sr, threads, feeders, device, errors, files_per_submit, stats, est)


def get_cqt_from_raw_bytes(raw_bytes, **kwargs):
    """One file's (rows, sr), as get_cqt_batch."""
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return get_cqt_batch([raw_bytes], **kwargs)[0]


def get_chroma_cqt_from_raw_bytes(raw_bytes, **kwargs):
    """One file's (rows, sr), as get_chroma_cqt_batch."""
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return get_chroma_cqt_batch([raw_bytes], **kwargs)[0]
