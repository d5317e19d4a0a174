"""Fundamental frequency per frame from Ogg bytes, estimated on the GPU: a list of (f0, cmnd, sr) (get_f0_batch, YIN) or of
(f0, voiced_flag, voiced_prob, sr) (get_pyin_batch, pYIN: include/vorbis_synth_hip.h, "pyin", with tests/pyin_model.py as its
contract). ctypes onto libparseoggvorbis_amd.so (ogg_vorbis_pitch_corpus, ogg_vorbis_pyin_corpus). The estimator is YIN as librosa.yin computes it (librosa >= 0.10 defaults:
win_length = frame_length // 2, pad_mode="constant") on the mono signal y = get_pcm_batch(mono=True, sr=sr), after the optional
resampler and before anything is copied back: no PCM crosses the bus. The arithmetic is written out in include/vorbis_synth_hip.h
("pitch") and the float64 model in tests/pitch_model.py is the contract; parity with librosa itself is not claimed. Frame f lines
up with row f of get_spectral_batch(n_fft=frame_length, hop_length=hop_length).

Every argument is checked before the library is loaded."""
import ctypes as C
import math

import numpy as np

from . import _corpus
from ._corpus import HOST_LIB_PATH  # noqa: F401
from .pcm import TRIM_MAX_FRAME, U32_MAX, check_sr

PITCH_CENTER = 1  # VSYN_PITCH_CENTER
MIN_FRAME = 4


class PitchError(RuntimeError):
    pass


def _real(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise PitchError("%s must be a number, got %r" % (name, v))
    if not math.isfinite(float(v)):
        raise PitchError("%s must be finite, got %r" % (name, v))
    return float(v)


def pitch_spec(fmin, fmax, frame_length=2048, hop_length=None, trough_threshold=0.1, center=True):
    """Checks the arguments (include/vorbis_synth_hip.h, "pitch", step 10, as far as they can be without a file's rate) and returns
    the C spec (binding.PitchSpec): frame_length an integer in [4, 8192]; hop_length None (frame_length // 4) or an integer >= 1
    (that the C spec's uint32 holds); 0 < fmin < fmax, finite; 0 < trough_threshold <= 1; center a bool."""
    from .binding import PitchSpec
    for name, v, lo, hi in (("frame_length", frame_length, MIN_FRAME, TRIM_MAX_FRAME), ("hop_length", hop_length, 1, U32_MAX)):
        if name == "hop_length" and v is None:
            continue
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise PitchError("%s must be an integer, got %r" % (name, v))
        if not lo <= int(v) <= hi:
            raise PitchError("%s must be in [%d, %d], got %d" % (name, lo, hi, int(v)))
    if not isinstance(center, (bool, np.bool_)):
        raise PitchError("center must be a bool, got %r" % (center,))
    lo, hi, thr = _real("fmin", fmin), _real("fmax", fmax), _real("trough_threshold", trough_threshold)
    if not 0.0 < lo < hi:
        raise PitchError("need 0 < fmin < fmax, got fmin %r, fmax %r" % (fmin, fmax))
    if not 0.0 < thr <= 1.0:
        raise PitchError("trough_threshold must be in (0, 1], got %r" % (trough_threshold,))
    L = int(frame_length)
    H = L // 4 if hop_length is None else int(hop_length)
    return PitchSpec(L, H, PITCH_CENTER if center else 0, 0, lo, hi, thr)


_load = _corpus.load


class PyinError(RuntimeError):
    pass


PYIN_MAX_THRESHOLDS = 1024
PYIN_MAX_STATES = 4096  # VSYN_PYIN_MAX_STATES


def _beta_cdf_int(x, a, b):
    """I_x(a, b) for integers a, b >= 1 by the exact binomial sum: sum_{j=a}^{a+b-1} C(a+b-1, j) x^j (1-x)^(a+b-1-j)."""
    n = a + b - 1
    return math.fsum(math.comb(n, j) * x ** j * (1.0 - x) ** (n - j) for j in range(a, n + 1))


def beta_probs(n_thresholds, beta_parameters=(2, 18)):
    """The table of "pyin" step 3: the differences of the Beta(a, b) distribution function at numpy.linspace(0, 1, N + 1), float64
    (N,). Integer parameters take the exact binomial sum; others need scipy.special.betainc, imported here and not with the package."""
    a, b = beta_parameters
    x = np.linspace(0.0, 1.0, n_thresholds + 1)
    if all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in (a, b)):
        cdf = np.array([0.0] + [_beta_cdf_int(float(t), int(a), int(b)) for t in x[1:-1]] + [1.0])
    else:
        try:
            from scipy.special import betainc
        except ImportError as e:
            raise PyinError("beta_parameters %r are not integers: that needs scipy, which is missing (%s)" % (beta_parameters, e))
        cdf = np.asarray(betainc(float(a), float(b), x), np.float64)
    cdf = np.maximum.accumulate(np.clip(cdf, 0.0, 1.0))  # (a rounding may put a sum an ulp above its neighbour: no weight is negative)
    return np.ascontiguousarray(np.diff(cdf), np.float64)


def _pyin_real(name, v):
    try:
        return _real(name, v)
    except PitchError as e:
        raise PyinError(str(e))


def pyin_spec(fmin, fmax, frame_length=2048, hop_length=None, n_thresholds=100, beta_parameters=(2, 18), boltzmann_parameter=2, resolution=0.1,
              max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01, center=True):
    """Checks the arguments (include/vorbis_synth_hip.h, "pyin", step 10, as far as they can be without a file's rate) and returns the
    C spec (binding.PyinSpec, which keeps its table alive): frame_length, hop_length, fmin, fmax and center as for pitch_spec;
    n_thresholds an integer in [1, 1024]; beta_parameters two numbers above 0; boltzmann_parameter > 0; 0 < resolution < 1;
    max_transition_rate > 0; 0 < switch_prob < 1; 0 <= no_trough_prob <= 1; 2 B <= 4096 states."""
    from .binding import PyinSpec
    try:
        base = pitch_spec(fmin, fmax, frame_length, hop_length, 1.0, center)
    except PitchError as e:
        raise PyinError(str(e))
    if isinstance(n_thresholds, (bool, np.bool_)) or not isinstance(n_thresholds, (int, np.integer)) or not 1 <= int(n_thresholds) <= PYIN_MAX_THRESHOLDS:
        raise PyinError("n_thresholds must be an integer in [1, %d], got %r" % (PYIN_MAX_THRESHOLDS, n_thresholds))
    try:
        a, b = beta_parameters
    except (TypeError, ValueError):
        raise PyinError("beta_parameters must be two numbers, got %r" % (beta_parameters,))
    if not (_pyin_real("beta_parameters[0]", a) > 0.0 and _pyin_real("beta_parameters[1]", b) > 0.0):
        raise PyinError("beta_parameters must be above 0, got %r" % (beta_parameters,))
    lam, res, mtr = _pyin_real("boltzmann_parameter", boltzmann_parameter), _pyin_real("resolution", resolution), _pyin_real("max_transition_rate", max_transition_rate)
    sw, ntp = _pyin_real("switch_prob", switch_prob), _pyin_real("no_trough_prob", no_trough_prob)
    if not lam > 0.0:
        raise PyinError("boltzmann_parameter must be above 0, got %r" % (boltzmann_parameter,))
    if not 0.0 < res < 1.0:
        raise PyinError("resolution must be in (0, 1), got %r" % (resolution,))
    if not mtr > 0.0:
        raise PyinError("max_transition_rate must be above 0, got %r" % (max_transition_rate,))
    if not 0.0 < sw < 1.0:
        raise PyinError("switch_prob must be in (0, 1), got %r" % (switch_prob,))
    if not 0.0 <= ntp <= 1.0:
        raise PyinError("no_trough_prob must be in [0, 1], got %r" % (no_trough_prob,))
    bins = math.floor(12 * math.ceil(1.0 / res) * math.log2(base.fmax / base.fmin)) + 1
    if 2 * bins > PYIN_MAX_STATES:
        raise PyinError("fmin %r, fmax %r and resolution %r give %d pitch bins: at most %d" % (fmin, fmax, resolution, bins, PYIN_MAX_STATES // 2))
    probs = beta_probs(int(n_thresholds), (a, b))
    if not (np.isfinite(probs).all() and (probs >= 0.0).all()):
        raise PyinError("beta_parameters %r give a table that is not finite and >= 0" % (beta_parameters,))
    spec = PyinSpec(base.frame_length, base.hop_length, base.options, int(n_thresholds), base.fmin, base.fmax, lam, res, mtr, sw, ntp, probs.ctypes.data)
    spec.probs = probs  # (the pointer's owner)
    return spec


def get_pyin_batch(list_of_bytes, fmin, fmax, frame_length=2048, hop_length=None, n_thresholds=100, beta_parameters=(2, 18), boltzmann_parameter=2,
                   resolution=0.1, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01, fill_na=np.nan, center=True, sr=None,
                   threads=0, feeders=0, device=0, errors="raise", files_per_submit=64, stats=None):
    """pYIN of many Ogg Vorbis files in one corpus run: a list of (f0, voiced_flag, voiced_prob, sr) tuples, what librosa.pyin(y,
    fmin=fmin, fmax=fmax, sr=sr, frame_length=frame_length, hop_length=hop_length, n_thresholds=n_thresholds, ..., fill_na=fill_na,
    center=center) computes for the mono signal y = get_pcm_batch(mono=True, sr=sr): f0 float32 (F,) in Hz, voiced_flag bool (F,),
    voiced_prob float32 (F,), and the rate they were computed at. fill_na replaces f0 on unvoiced frames (NaN by default, or a
    number); fill_na=None keeps the decoded bin's frequency there. hop_length=None means frame_length // 4. sr, errors and stats as
    for get_pcm_batch. A file whose rate does not fit (as for get_f0_batch, or an even transition width at that rate) fails alone,
    and so does a file with an Inf or NaN sample: errors="raise" raises PyinError naming the first such file, errors="return" puts
    the PyinError in its slot."""
    _corpus.check_errors(errors)
    target = check_sr(sr, PyinError)
    if fill_na is not None:
        if isinstance(fill_na, (bool, np.bool_)) or not isinstance(fill_na, (int, float, np.integer, np.floating)):
            raise PyinError("fill_na must be None or a number, got %r" % (fill_na,))
    spec = pyin_spec(fmin, fmax, frame_length, hop_length, n_thresholds, beta_parameters, boltzmann_parameter, resolution, max_transition_rate,
                     switch_prob, no_trough_prob, center)
    lib = _load()
    n = len(list_of_bytes)
    counts = np.zeros(max(n, 1), np.uint64)
    frames = np.zeros(max(n, 1), np.uint64)
    rates = np.zeros(max(n, 1), np.uint32)

    def build(i, p):
        rows = _corpus.copy_into(np.zeros((int(counts[i]), 3), np.float32), p)
        f0, voiced = np.ascontiguousarray(rows[:, 0]), rows[:, 1] > 0.5
        if fill_na is not None:
            f0[~voiced] = fill_na
        return f0, voiced, np.ascontiguousarray(rows[:, 2]), int(rates[i])

    return _corpus.run(lib, lib.ogg_vorbis_pyin_corpus, list_of_bytes, (threads, feeders, files_per_submit, device, target, C.byref(spec)),
                       (counts, frames, rates), build, PyinError, errors, "pyin", stats)


def get_pyin_from_raw_bytes(raw_bytes, fmin, fmax, **kwargs):
    """One file's (f0, voiced_flag, voiced_prob, sr), as get_pyin_batch."""
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return get_pyin_batch([raw_bytes], fmin, fmax, **kwargs)[0]


def get_f0_batch(list_of_bytes, fmin, fmax, frame_length=2048, hop_length=None, trough_threshold=0.1, center=True, sr=None, threads=0,
                 feeders=0, device=0, errors="raise", files_per_submit=64, stats=None):
    """The fundamental frequency of many Ogg Vorbis files in one corpus run: a list of (f0, cmnd, sr) tuples. f0 is float32 (F,), in
    Hz, what librosa.yin(y, fmin=fmin, fmax=fmax, sr=sr, frame_length=frame_length, hop_length=hop_length,
    trough_threshold=trough_threshold, center=center) computes for the mono signal y = get_pcm_batch(mono=True, sr=sr); cmnd is
    float32 (F,), the cumulative-mean-normalised difference at the chosen lag (small: periodic; near 1: not), which librosa
    discards and a caller thresholds for voicing; sr is the rate both were computed at. hop_length=None means frame_length // 4.
    sr, errors and stats as for get_pcm_batch. A file whose rate does not fit (fmax above sr / 2, or fewer than two lags between
    sr / fmax and min(sr / fmin, frame_length - frame_length // 2 - 1)) fails alone, and so does a file with an Inf or NaN sample:
    errors="raise" raises PitchError naming the first such file, errors="return" puts the PitchError in its slot."""
    _corpus.check_errors(errors)
    target = check_sr(sr, PitchError)
    spec = pitch_spec(fmin, fmax, frame_length, hop_length, trough_threshold, center)
    lib = _load()
    n = len(list_of_bytes)
    counts = np.zeros(max(n, 1), np.uint64)
    frames = np.zeros(max(n, 1), np.uint64)
    rates = np.zeros(max(n, 1), np.uint32)

    def build(i, p):
        rows = _corpus.copy_into(np.zeros((int(counts[i]), 2), np.float32), p)
        return np.ascontiguousarray(rows[:, 0]), np.ascontiguousarray(rows[:, 1]), int(rates[i])

    return _corpus.run(lib, lib.ogg_vorbis_pitch_corpus, list_of_bytes, (threads, feeders, files_per_submit, device, target, C.byref(spec)),
                       (counts, frames, rates), build, PitchError, errors, "pitch", stats)


def get_f0_from_raw_bytes(raw_bytes, fmin, fmax, **kwargs):
    """One file's (f0, cmnd, sr), as get_f0_batch."""
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return get_f0_batch([raw_bytes], fmin, fmax, **kwargs)[0]
