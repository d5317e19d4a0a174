"""Spectral front-end features computed on the GPU from Ogg bytes: mel power, log-mel, dB-mel and MFCC matrices
(frames, dim) float32, and the linear spectra they are built from (magnitude / power, dB, complex STFT), from the decoded PCM while it is still on the device (no PCM crosses the bus). ctypes onto
libparseoggvorbis_amd.so (ogg_vorbis_spectral_corpus_sr); the semantics are documented in include/vorbis_synth_hip.h ("spectral
features"). They follow librosa's documented defaults (librosa >= 0.10); parity with librosa itself has not been verified, the
float64 model in tests/spectral_model.py is the contract the device is tested against.

Every argument is checked before the library is loaded. 25 ms / 10 ms at 44.1 kHz: n_fft=1102, hop_length=441. sr=None computes
each file's matrix at its own rate; an integer sr resamples every file's PCM to it on the device first (parseoggvorbis_amd/pcm.py,
scipy.signal.resample_poly's arithmetic), so that one mel table serves the whole batch. delta / normalize finish the rows on the
device as well (include/vorbis_synth_hip.h, "spectral post-processing"): librosa.feature.delta's columns, then per-column mean or
mean / variance normalisation; tests/spectral_post_model.py is their float64 model. peak_normalize / preemphasis condition the mono
waveform on the device in front of the STFT (include/vorbis_synth_hip.h, "PCM conditioning"; model: tests/condition_model.py), and
trim_db cuts its silent head and tail in front of both ("PCM trimming"; model: tests/trim_model.py), or split_db every silent
stretch ("PCM splitting"; model: tests/split_model.py). pcen=True turns the rows of "mel_power" or "lin_power" into librosa.pcen's
on the device, between the spectral rows and delta / normalize ("PCEN"; model: tests/pcen_model.py). kind="chroma" / "tonnetz" give
librosa.feature.chroma_stft's pitch-class rows and librosa.feature.tonnetz's coordinates from them ("chroma"; model:
tests/chroma_model.py; ogg_vorbis_spectral_corpus_chroma). hpss="harmonic" / "percussive" turns the rows of "mel_power" or
"lin_power" into librosa.decompose.hpss's component (or its mask, or the median itself) on the device, between the spectral rows and
PCEN ("HPSS"; model: tests/hpss_model.py; ogg_vorbis_spectral_corpus_hpss)."""
import ctypes as C
import math

import numpy as np

from . import _corpus
from ._corpus import HOST_LIB_PATH  # noqa: F401

KINDS = {"mel_power": 1, "log_mel": 2, "mel_db": 3, "mfcc": 4, "lin_power": 5, "lin_db": 6, "stft": 7}
LINEAR_KINDS = (5, 6, 7)  # include/vorbis_synth_hip.h, "linear spectra": no filterbank, rows of n_fft / 2 + 1 bins
# include/vorbis_synth_hip.h, "chroma": rows of n_chroma pitch classes, and the 6 tonnetz coordinates from them. A table of their own:
# KINDS holds the kinds whose row width the spectral spec alone decides (vsyn_spectral_dim), these need the chroma arguments as well
CHROMA_KINDS = {"chroma": 8, "tonnetz": 9}
ALL_KINDS = dict(KINDS, **CHROMA_KINDS)  # what kind= accepts
CHROMA_NORMS = {None: 0, 1: 1, 2: 2, math.inf: 3}  # chroma_norm -> vsyn_spectral_chroma.norm
CHROMA_BASE_C, CHROMA_NO_OCT = 1, 2
MAX_N_CHROMA = 256
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
    file) and returns the C spec (binding.SpectralSpec). Every argument is checked for every kind, the linear kinds ("lin_power",
    "lin_db", "stft": "linear spectra" there) included, although the device reads no mel argument for those."""
    from .binding import SpectralSpec
    if kind not in ALL_KINDS:
        raise SpectralError("invalid spectral kind %r; supported kinds: %s" % (kind, ", ".join(sorted(ALL_KINDS))))
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
    if kind in ("mel_db", "mfcc", "lin_db") and not amin > 0:
        raise SpectralError("amin must be > 0, got %r" % amin)
    if kind in ("mel_db", "mfcc", "lin_db") and not top_db >= 0:
        raise SpectralError("top_db must be >= 0 (or None), got %r" % top_db)
    opts = (OPT_CENTER if center else 0) | (OPT_HTK if htk else 0) | (OPT_NO_NORM if norm is None else 0)
    return SpectralSpec(ALL_KINDS[kind], opts, n_fft, hop_length, win_length, n_mels, n_mfcc if kind == "mfcc" else 0, int(power),
                        fmin, fmax, log_floor, amin, top_db)


def chroma_spec(n_chroma=12, tuning=0.0, chroma_norm=math.inf, ctroct=5.0, octwidth=2.0, base_c=True):
    """Checks the chroma arguments (include/vorbis_synth_hip.h, "chroma", step 6) and returns the C struct (binding.SpectralChroma).
    chroma_norm: numpy.inf (max), 1, 2 or None; octwidth=None: no octave weighting. tuning is a number here; librosa's tuning=None
    (estimate_tuning first) is get_spectral_batch(tuning="estimate"), and None itself stays refused."""
    from .binding import SpectralChroma
    n_chroma = _int("n_chroma", n_chroma)
    if not 1 <= n_chroma <= MAX_N_CHROMA:
        raise SpectralError("n_chroma must be in [1, %d], got %d" % (MAX_N_CHROMA, n_chroma))
    if isinstance(chroma_norm, bool) or not (chroma_norm is None or (isinstance(chroma_norm, (int, float, np.integer, np.floating))
                                                                     and chroma_norm in (1, 2, math.inf))):
        raise SpectralError("chroma_norm must be numpy.inf, 1, 2 or None, got %r" % (chroma_norm,))
    norm = CHROMA_NORMS[None if chroma_norm is None else (math.inf if chroma_norm == math.inf else int(chroma_norm))]
    vals = {}
    if tuning is None:
        raise SpectralError("tuning must be a finite number, got None (librosa's tuning=None is tuning=\"estimate\" in get_spectral_batch)")
    for name, v in (("tuning", tuning), ("ctroct", ctroct), ("octwidth", octwidth)):
        if name == "octwidth" and v is None:
            vals[name] = 0.0
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
            raise SpectralError("%s must be a finite number%s, got %r" % (name, " (or None)" if name == "octwidth" else "", v))
        vals[name] = float(v)
    if octwidth is not None and not vals["octwidth"] > 0.0:
        raise SpectralError("octwidth must be > 0 (or None), got %r" % (octwidth,))
    if not isinstance(base_c, (bool, np.bool_)):
        raise SpectralError("base_c must be True or False, got %r" % (base_c,))
    opts = (CHROMA_BASE_C if base_c else 0) | (CHROMA_NO_OCT if octwidth is None else 0)
    return SpectralChroma(n_chroma, norm, opts, 0, vals["tuning"], vals["ctroct"], vals["octwidth"])


def spec_dim(spec, chroma=None):
    """Columns of a row under spec (the one formula on the Python side, usable before the library loads): n_mfcc for "mfcc",
    n_fft / 2 + 1 for "lin_power" and "lin_db", twice that for "stft" (re, im interleaved), n_mels for the other mel kinds; 0 for an
    unknown kind. Without chroma it is vsyn_spectral_dim, which answers 0 for "chroma" and "tonnetz" (their width is a chroma
    argument); with chroma (chroma_spec(...); chroma_spec() for the defaults) it is vsyn_spectral_chroma_dim: n_chroma and 6."""
    if spec.kind == KINDS["mfcc"]:
        return spec.n_mfcc
    if spec.kind in CHROMA_KINDS.values():
        return 0 if chroma is None else chroma.n_chroma if spec.kind == CHROMA_KINDS["chroma"] else 6
    if spec.kind in LINEAR_KINDS:
        return (spec.n_fft // 2 + 1) * (2 if spec.kind == KINDS["stft"] else 1)
    return spec.n_mels if spec.kind in KINDS.values() else 0


NORM_NONE, NORM_MEAN, NORM_MEAN_VAR = 0, 1, 2
STATS_SEGMENT, STATS_GIVEN = 0, 1
MAX_DELTA_WIDTH = 65


def post_spec(dim, delta=0, delta_width=9, normalize=None, std_floor=1e-5):
    """Checks the post-processing arguments (include/vorbis_synth_hip.h, "spectral post-processing", step 4) for rows of dim columns.
    Returns (C post spec, D_out, arrays the spec points into: keep them alive during the call), or (None, dim, ()) when the stage is
    off (delta=0, normalize=None). normalize: None, "mean", "mean_var" (per file), or (mean, std) of D_out entries each, std None
    for the mean alone."""
    from .binding import SpectralPost
    delta = _int("delta", delta)
    delta_width = _int("delta_width", delta_width)
    if not 0 <= delta <= 2:
        raise SpectralError("delta must be 0, 1 or 2, got %d" % delta)
    if not 3 <= delta_width <= MAX_DELTA_WIDTH or delta_width % 2 == 0:
        raise SpectralError("delta_width must be odd and in [3, %d], got %d" % (MAX_DELTA_WIDTH, delta_width))
    if isinstance(std_floor, bool) or not isinstance(std_floor, (int, float, np.integer, np.floating)):
        raise SpectralError("std_floor must be a number, got %r" % (std_floor,))
    std_floor = float(std_floor)
    if not (math.isfinite(std_floor) and std_floor > 0.0):
        raise SpectralError("std_floor must be finite and > 0, got %r" % std_floor)
    dout = dim * (1 + delta)
    norm, stats, keep = NORM_NONE, STATS_SEGMENT, ()
    if isinstance(normalize, str) and normalize in ("mean", "mean_var"):
        norm = NORM_MEAN if normalize == "mean" else NORM_MEAN_VAR
    elif isinstance(normalize, tuple) and len(normalize) == 2 and normalize[0] is not None:
        stats = STATS_GIVEN
        norm = NORM_MEAN if normalize[1] is None else NORM_MEAN_VAR
        vecs = []
        for name, v in (("mean", normalize[0]), ("std", normalize[1])):
            if v is None:
                continue
            try:
                a = np.ascontiguousarray(v, dtype=np.float32)
            except (TypeError, ValueError):
                raise SpectralError("normalize: %s must be an array of %d numbers" % (name, dout))
            if a.shape != (dout,):
                raise SpectralError("normalize: %s must have %d entries (dim %d x (1 + delta %d)), got shape %r"
                                    % (name, dout, dim, delta, a.shape))
            if not np.isfinite(a).all():
                raise SpectralError("normalize: %s must be finite" % name)
            vecs.append(a)
        keep = tuple(vecs)
    elif normalize is not None:
        raise SpectralError("normalize must be None, 'mean', 'mean_var' or a tuple (mean, std), got %r" % (normalize,))
    if delta == 0 and norm == NORM_NONE:
        return None, dim, ()
    post = SpectralPost(delta, delta_width, norm, stats, std_floor, keep[0].ctypes.data if keep else None,
                        keep[1].ctypes.data if len(keep) > 1 else None)
    return post, dout, keep


PCEN_KINDS = ("mel_power", "lin_power")  # include/vorbis_synth_hip.h, "PCEN": the kinds whose rows cannot be negative


def _number(name, v, positive):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise SpectralError("%s must be a number, got %r" % (name, v))
    v = float(v)
    if not (math.isfinite(v) and (v > 0.0 if positive else v >= 0.0)):
        raise SpectralError("%s must be finite and %s 0, got %r" % (name, ">" if positive else ">=", v))
    return v


def pcen_spec(gain=0.98, bias=2.0, power=0.5, time_constant=0.4, eps=1e-6, b=None, scale=1.0):
    """Checks the PCEN arguments (include/vorbis_synth_hip.h, "PCEN", step 6) and returns the C spec (binding.SpectralPcen). b=None:
    the coefficient is derived per file from time_constant, the rate its rows are computed at and hop_length (encoded as 0)."""
    from .binding import SpectralPcen
    gain, bias, power = _number("pcen_gain", gain, False), _number("pcen_bias", bias, False), _number("pcen_power", power, False)
    time_constant, eps = _number("pcen_time_constant", time_constant, True), _number("pcen_eps", eps, True)
    scale = _number("pcen_scale", scale, True)
    if b is not None:
        b = _number("pcen_b", b, True)
        if b > 1.0:
            raise SpectralError("pcen_b must be in (0, 1] (or None), got %r" % b)
    return SpectralPcen(gain, bias, power, time_constant, eps, 0.0 if b is None else b, scale)


HPSS_KINDS = PCEN_KINDS  # include/vorbis_synth_hip.h, "HPSS": the same two kinds
HPSS_COMPONENTS = {"harmonic": 0, "percussive": 1}
HPSS_OUTPUTS = {"component": 0, "mask": 1, "median": 2}
MAX_HPSS_KERNEL = 63


def _pair(name, v):
    """A number, or a (harmonic, percussive) pair of them."""
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise SpectralError("%s must be one value or a (harmonic, percussive) pair, got %r" % (name, v))
        return v[0], v[1]
    return v, v


def hpss_spec(component="harmonic", kernel_size=31, power=2.0, margin=1.0, output="component"):
    """Checks the HPSS arguments (include/vorbis_synth_hip.h, "HPSS", step 5) and returns the C spec (binding.SpectralHpss).
    kernel_size and margin: one value or a (harmonic, percussive) pair; kernel sizes odd and in [1, 63]; margins finite and >= 1;
    power > 0, numpy.inf for the hard mask."""
    from .binding import SpectralHpss
    if not isinstance(component, str) or component not in HPSS_COMPONENTS:
        raise SpectralError("hpss must be None, %s, got %r" % (" or ".join(repr(k) for k in HPSS_COMPONENTS), component))
    if not isinstance(output, str) or output not in HPSS_OUTPUTS:
        raise SpectralError("hpss_output must be %s, got %r" % (" or ".join(repr(k) for k in HPSS_OUTPUTS), output))
    ks = [_int("hpss_kernel_size", k) for k in _pair("hpss_kernel_size", kernel_size)]
    for k in ks:
        if not (1 <= k <= MAX_HPSS_KERNEL and k % 2 == 1):
            raise SpectralError("hpss_kernel_size must be odd and in [1, %d], got %r" % (MAX_HPSS_KERNEL, k))
    ms = [_number("hpss_margin", m, True) for m in _pair("hpss_margin", margin)]
    for m in ms:
        if m < 1.0:
            raise SpectralError("hpss_margin must be >= 1, got %r" % m)
    if isinstance(power, bool) or not isinstance(power, (int, float, np.integer, np.floating)) or not float(power) > 0.0:
        raise SpectralError("hpss_power must be a number > 0 (numpy.inf: the hard mask), got %r" % (power,))
    return SpectralHpss(ks[0], ks[1], HPSS_COMPONENTS[component], HPSS_OUTPUTS[output], float(power), ms[0], ms[1])


# the arguments of get_spectral_batch that checked_specs reads, in the order it unpacks them
_CHECKED = ("errors", "sr", "kind", "n_fft", "hop_length", "win_length", "n_mels", "fmin", "fmax", "htk", "norm", "center",
            "power", "log_floor", "amin", "top_db", "n_mfcc", "n_chroma", "tuning", "chroma_norm", "ctroct", "octwidth", "base_c",
            "delta", "delta_width", "normalize", "std_floor", "pcen_gain", "pcen_bias", "pcen_power", "pcen_time_constant",
            "pcen_eps", "pcen_b", "pcen_scale", "pcen", "hpss", "hpss_kernel_size", "hpss_power", "hpss_margin", "hpss_output",
            "peak_normalize", "preemphasis", "trim_db", "trim_frame_length", "trim_hop_length", "trim_index", "split_db",
            "split_frame_length", "split_hop_length", "split_index", "loudness_normalize", "loudness")


def checked_specs(a):
    """Every check of get_spectral_batch's arguments, a being the dict of them (its locals()), before anything is loaded: the C specs of
    the stages and the width of the rows. Shared with rhythm.py, whose entries forward the same arguments."""
    from types import SimpleNamespace
    (errors, sr, kind, n_fft, hop_length, win_length, n_mels, fmin, fmax, htk, norm, center, power, log_floor, amin, top_db,
     n_mfcc, n_chroma, tuning, chroma_norm, ctroct, octwidth, base_c, delta, delta_width, normalize, std_floor, pcen_gain,
     pcen_bias, pcen_power, pcen_time_constant, pcen_eps, pcen_b, pcen_scale, pcen, hpss, hpss_kernel_size, hpss_power,
     hpss_margin, hpss_output, peak_normalize, preemphasis, trim_db, trim_frame_length, trim_hop_length, trim_index, split_db,
     split_frame_length, split_hop_length, split_index, loudness_normalize, loudness) = (a[k] for k in _CHECKED)
    _corpus.check_errors(errors)
    from .pcm import check_sr, cond_spec, loudness_args, split_spec, trim_spec
    target = check_sr(sr, SpectralError)
    spec = spectral_spec(kind, n_fft, hop_length, win_length, n_mels, fmin, fmax, htk, norm, center, power, log_floor, amin, top_db,
                         n_mfcc)
    est = None
    if isinstance(tuning, str) and tuning == "estimate":  # librosa's tuning=None: each file's own estimate first (tuning.py)
        if "tuning_resolution" not in a:
            raise SpectralError("tuning='estimate' is available in get_spectral_batch only")
        if kind not in CHROMA_KINDS:
            raise SpectralError("tuning='estimate' is for kind %s, not %r" % (" or ".join(repr(k) for k in CHROMA_KINDS), kind))
        if hpss is not None:
            raise SpectralError("tuning='estimate' is not available with hpss")
        from .tuning import TuningError, tuning_spec
        try:
            est = tuning_spec(a["tuning_fmin"], a["tuning_fmax"], a["tuning_threshold"], a["tuning_resolution"],
                              n_chroma if isinstance(n_chroma, (int, np.integer)) and not isinstance(n_chroma, bool) and 1 <= n_chroma <= 256 else 12)
        except TuningError as e:
            raise SpectralError("tuning='estimate': tuning_%s" % e) from None
        tuning = 0.0
    chroma = chroma_spec(n_chroma, tuning, chroma_norm, ctroct, octwidth, base_c)
    post, dim, keep = post_spec(spec_dim(spec, chroma), delta, delta_width, normalize, std_floor)
    if post is not None and spec.kind in LINEAR_KINDS:
        raise SpectralError("delta / normalize are not available for the linear kind %r (rows of %d columns; the post stage holds 256)"
                            % (kind, dim))
    pc = pcen_spec(pcen_gain, pcen_bias, pcen_power, pcen_time_constant, pcen_eps, pcen_b, pcen_scale)
    if not isinstance(pcen, (bool, np.bool_)):
        raise SpectralError("pcen must be True or False, got %r" % (pcen,))
    if pcen and kind not in PCEN_KINDS:
        raise SpectralError("pcen is not available for kind %r: it takes the rows of %s" % (kind, " or ".join(PCEN_KINDS)))
    hp = hpss_spec("harmonic" if hpss is None else hpss, hpss_kernel_size, hpss_power, hpss_margin, hpss_output)
    if hpss is not None and kind not in HPSS_KINDS:
        raise SpectralError("hpss is not available for kind %r: it takes the rows of %s" % (kind, " or ".join(HPSS_KINDS)))
    if hpss is not None and pcen and hpss_output != "component":
        raise SpectralError("pcen takes the hpss component, not hpss_output=%r" % (hpss_output,))
    cond = cond_spec(peak_normalize, preemphasis, SpectralError)
    trim = trim_spec(trim_db, trim_frame_length, trim_hop_length, trim_index, SpectralError)
    split = split_spec(split_db, split_frame_length, split_hop_length, split_index, trim, SpectralError)
    loud = loudness_args(loudness_normalize, loudness, cond, SpectralError)
    return SimpleNamespace(target=target, spec=spec, chroma=chroma, post=post, dim=dim, keep=keep, pc=pc, hp=hp, cond=cond, trim=trim, split=split,
                           loud=loud, est=est)


_load = _corpus.load


def get_spectral_batch(list_of_bytes, kind="log_mel", n_fft=2048, hop_length=512, win_length=None, n_mels=128, fmin=0.0, fmax=None,
                       htk=False, norm="slaney", center=True, power=2.0, log_floor=1e-3, amin=1e-10, top_db=80.0, n_mfcc=20,
                       threads=0, feeders=0, device=0, errors="raise", files_per_submit=64, stats=None, sr=None, delta=0, delta_width=9,
                       normalize=None, std_floor=1e-5, peak_normalize=False, preemphasis=None, trim_db=None, trim_frame_length=2048,
                       trim_hop_length=512, trim_index=None, split_db=None, split_frame_length=2048, split_hop_length=512, split_index=None,
                       pcen=False, pcen_gain=0.98, pcen_bias=2.0, pcen_power=0.5, pcen_time_constant=0.4, pcen_eps=1e-6, pcen_b=None,
                       pcen_scale=1.0, loudness_normalize=None, loudness=None, n_chroma=12, tuning=0.0, chroma_norm=math.inf, ctroct=5.0,
                       octwidth=2.0, base_c=True, hpss=None, hpss_kernel_size=31, hpss_power=2.0, hpss_margin=1.0, hpss_output="component",
                       tuning_resolution=0.01, tuning_fmin=150.0, tuning_fmax=4000.0, tuning_threshold=0.1, tunings=None):
    """Spectral matrices of many Ogg Vorbis files in one corpus run: a list of float32 arrays (frames, dim), dim = n_mfcc for
    "mfcc", n_mels for the other mel kinds. The linear kinds have no filterbank: "lin_power" is |X|^power and "lin_db" its dB image
    (amin, top_db as for "mel_db"; librosa.amplitude_to_db(|X|, amin=a) is power=2, amin=a*a), both (frames, n_fft / 2 + 1);
    "stft" is the complex STFT itself, complex64 arrays (frames, n_fft / 2 + 1) with numpy.fft.rfft's sign. They take neither
    delta nor normalize (SpectralError before anything is loaded) and compose with sr, peak_normalize / preemphasis, trim_db and
    split_db like the mel kinds; their rows are n_fft / 2 + 1 floats wide, so files_per_submit bounds the memory of a run. errors="raise": the first failed file raises SpectralError naming it; errors="return": its entry
    is the SpectralError. stats (optional list) receives the run's 8 corpus statistics. sr=None: each file at its own rate;
    an integer: every file resampled to sr on the device, and the mel table and the fmin / fmax check use sr.
    delta = 1 or 2 appends librosa.feature.delta's columns of that many orders (Savitzky-Golay over delta_width frames; a file
    with fewer frames than delta_width fails alone); normalize = "mean" / "mean_var" normalises every column per file, a tuple
    (mean, std) with the caller's vectors (std None: mean only), dividing by max(std, std_floor). The arrays are then
    (frames, dim * (1 + delta)); with the defaults the stage is off and the rows are those of the spectral kernels.
    peak_normalize=True divides the mono signal (after the resampling) by its largest magnitude before the STFT, preemphasis=a
    (0 < a < 1) then filters it as z[t] = y[t] - a y[t-1] (get_pcm_batch(mono=True, ...) returns that signal); a file with an Inf
    or NaN sample fails alone under peak_normalize. With the defaults nothing is launched.
    trim_db=d cuts the silent head and tail of the mono signal first, as get_pcm_batch(mono=True, trim_db=d, ...) does (the peak, the
    pre-emphasis, the frames and "fewer frames than delta_width" are those of what is kept); trim_index (optional list) receives
    one (start, end) per file in samples of the (resampled) signal, None for a failed file and for every file with the stage off.
    split_db=d (instead of trim_db) removes every silent stretch of the mono signal first, as get_pcm_batch(mono=True, split_db=d,
    ...) does: the rows are those of the joined signal; split_index (optional list) receives one (n, 2) int64 array of (start, end)
    per file, None for a failed file and for every file with the stage off.
    pcen=True (kind "mel_power" or "lin_power" only; SpectralError before anything is loaded otherwise) replaces the rows by
    librosa.pcen(rows.T * pcen_scale, sr, hop_length, gain=pcen_gain, bias=pcen_bias, power=pcen_power,
    time_constant=pcen_time_constant, eps=pcen_eps, b=pcen_b, max_size=1).T on the device, in front of delta / normalize; sr is
    the rate the rows are computed at, so with sr=None the derived coefficient differs between files of different rates.
    librosa's documentation uses pcen_scale=2**31 for float PCM. With pcen=False the pcen_* arguments are still checked, nothing is
    launched and the call takes the entry points it took without them.
    loudness_normalize=L (LUFS in [-70, 0]; excludes peak_normalize) scales the mono signal to the integrated loudness L behind
    trim_db / split_db and in front of the pre-emphasis, as get_pcm_batch(mono=True, loudness_normalize=L, ...) does, and the rows are
    those of that signal; loudness (optional list) receives the measured LUFS per file. A file the measurement refuses (shorter than
    400 ms, silent, not finite, below 4000 Hz) fails alone. With loudness_normalize=None nothing is launched.
    kind="chroma" gives librosa.feature.chroma_stft's arithmetic (include/vorbis_synth_hip.h, "chroma"; model: tests/chroma_model.py):
    (frames, n_chroma) rows of the |X|^power spectrum (power=2 is chroma_stft's) projected on librosa.filters.chroma(sr, n_fft,
    n_chroma, tuning, ctroct, octwidth, base_c) and normalised per frame by chroma_norm (numpy.inf, 1, 2 or None); octwidth=None turns
    the octave weighting off. tuning is a number, or "estimate" (librosa's tuning=None; None itself stays refused): each file's tuning is
    estimated first on the device (parseoggvorbis_amd/tuning.py, "tuning estimation" in the header) from the signal the chroma kernel
    sees, at this call's n_fft, hop_length, win_length, center and power, with tuning_fmin, tuning_fmax, tuning_threshold,
    tuning_resolution and bins_per_octave = n_chroma; the rows are those of the same call with that number, bit for bit, and tunings
    (optional list) receives it per file, None for a failed file and for every file when tuning is a number. kind="tonnetz" gives
    librosa.feature.tonnetz(chroma=those rows): (frames, 6). A frame that holds an Inf or NaN sample is all NaN. Both take delta /
    normalize and every PCM stage like the mel kinds, and refuse pcen. The chroma arguments are checked for every kind.
    hpss="harmonic" / "percussive" (kind "mel_power" or "lin_power" only; SpectralError before anything is loaded otherwise) replaces
    the rows by that component of librosa.decompose.hpss(rows.T, kernel_size=hpss_kernel_size, power=hpss_power, margin=hpss_margin).T
    on the device (include/vorbis_synth_hip.h, "HPSS"; model: tests/hpss_model.py), in front of pcen and delta / normalize:
    hpss_kernel_size and hpss_margin are one value or a (harmonic, percussive) pair, the sizes odd and in [1, 63], the medians
    reflect at a file's first and last frame and at bin 0 and the last bin. hpss_output="mask" returns the soft mask instead and
    "median" the median-filtered rows themselves (along time for "harmonic", along bins for "percussive"); pcen takes neither of
    those two. With hpss=None the hpss_* arguments are still checked, nothing is launched and the call takes the entry points it took
    without them."""
    from .pcm import give_loudness, give_split_index, give_trim_index
    c = checked_specs(dict(locals()))
    target, spec, chroma, post, dim, pc, hp = c.target, c.spec, c.chroma, c.post, c.dim, c.pc, c.hp
    cond, trim, split, loud = c.cond, c.trim, c.split, c.loud
    if tunings is not None and not isinstance(tunings, list):
        raise SpectralError("tunings must be a list (or None), got %r" % (tunings,))
    lib = _load()
    counts = np.zeros(len(list_of_bytes), np.uint64)
    is_chroma = kind in CHROMA_KINDS
    if loud is not None or is_chroma or hpss is not None:  # the entries with every stage's spec, the normaliser's among them (NULL: off); a chroma kind: with the chroma parameters
        from .binding import LOUDNESS_RECORD_DTYPE
        n = len(list_of_bytes)
        ib = _corpus.IntervalBuffers(lib, n)
        joined, bounds = np.zeros(max(n, 1), np.uint64), np.zeros((max(n, 1), 2), np.uint64)
        records = np.zeros(max(n, 1), LOUDNESS_RECORD_DTYPE)
        gate = split if split is not None else trim
        tail, est_out = (), ()
        try:
            if hpss is not None:  # the chroma entry with the HPSS spec behind the rate (its kinds read no chroma parameters)
                fn, head, mid = lib.ogg_vorbis_spectral_corpus_hpss, (None,), (C.byref(hp),)
            elif is_chroma and c.est is not None:
                fn, head, mid = lib.ogg_vorbis_spectral_corpus_chroma_est, (C.byref(chroma),), ()
                tail, est_out = (C.byref(c.est),), (np.zeros(max(n, 1), np.float64),)
            elif is_chroma:
                fn, head, mid = lib.ogg_vorbis_spectral_corpus_chroma, (C.byref(chroma),), ()
            else:
                fn, head, mid = lib.ogg_vorbis_spectral_corpus_loud, (), ()
            res = _corpus.run(lib, fn, list_of_bytes,
                              (threads, feeders, files_per_submit, device, C.byref(spec)) + head + (target,) + mid +
                              (C.byref(pc) if pcen else None,
                               None if post is None else C.byref(post), C.byref(cond) if cond.options else None,
                               None if gate is None else C.byref(gate), int(split is not None), None if loud is None else C.byref(loud)) + tail,
                              (counts, bounds, joined, ib.ptrs, ib.counts, records) + est_out,
                              lambda i, p: _corpus.copy_into(np.zeros((int(counts[i]), dim), np.float32), p), SpectralError, errors,
                              "spectral", stats)
            give_split_index(split_index, ib if split is not None else None, res)
        finally:
            ib.free()
        give_trim_index(trim_index, bounds[:n] if trim is not None else None, res)
        give_loudness(loudness, records if loud is not None else None, res)
        if tunings is not None:
            tunings[:] = [float(est_out[0][i]) if est_out and isinstance(r, np.ndarray) else None for i, r in enumerate(res)]
        return _finish(spec, res)
    if tunings is not None:
        tunings[:] = [None] * len(list_of_bytes)
    give_loudness(loudness, None, [None] * len(list_of_bytes))
    if pcen:  # the one entry with every stage's spec (NULL: off)
        n = len(list_of_bytes)
        ib = _corpus.IntervalBuffers(lib, n)
        joined, bounds = np.zeros(max(n, 1), np.uint64), np.zeros((max(n, 1), 2), np.uint64)
        gate = split if split is not None else trim
        try:
            res = _corpus.run(lib, lib.ogg_vorbis_spectral_corpus_pcen, list_of_bytes,
                              (threads, feeders, files_per_submit, device, C.byref(spec), target, C.byref(pc), None if post is None else C.byref(post),
                               C.byref(cond) if cond.options else None, None if gate is None else C.byref(gate), int(split is not None)),
                              (counts, bounds, joined, ib.ptrs, ib.counts),
                              lambda i, p: _corpus.copy_into(np.zeros((int(counts[i]), dim), np.float32), p), SpectralError, errors,
                              "spectral", stats)
            give_split_index(split_index, ib if split is not None else None, res)
        finally:
            ib.free()
        give_trim_index(trim_index, bounds[:n] if trim is not None else None, res)
        return _finish(spec, res)
    if split is not None:
        ib = _corpus.IntervalBuffers(lib, len(list_of_bytes))
        joined = np.zeros(max(len(list_of_bytes), 1), np.uint64)
        try:
            res = _corpus.run(lib, lib.ogg_vorbis_spectral_corpus_split, list_of_bytes,
                              (threads, feeders, files_per_submit, device, C.byref(spec), target, None if post is None else C.byref(post),
                               C.byref(cond) if cond.options else None, C.byref(split)), (counts, joined, ib.ptrs, ib.counts),
                              lambda i, p: _corpus.copy_into(np.zeros((int(counts[i]), dim), np.float32), p), SpectralError, errors,
                              "spectral", stats)
            give_split_index(split_index, ib, res)
        finally:
            ib.free()
        give_trim_index(trim_index, None, res)
        return _finish(spec, res)
    give_split_index(split_index, None, [None] * len(list_of_bytes))
    if trim is not None:
        bounds = np.zeros((max(len(list_of_bytes), 1), 2), np.uint64)
        res = _corpus.run(lib, lib.ogg_vorbis_spectral_corpus_trim, list_of_bytes,
                          (threads, feeders, files_per_submit, device, C.byref(spec), target, None if post is None else C.byref(post),
                           C.byref(cond) if cond.options else None, C.byref(trim)), (counts, bounds),
                          lambda i, p: _corpus.copy_into(np.zeros((int(counts[i]), dim), np.float32), p), SpectralError, errors, "spectral",
                          stats)
        give_trim_index(trim_index, bounds[:len(list_of_bytes)], res)
        return _finish(spec, res)
    if cond.options:
        fn, extra = lib.ogg_vorbis_spectral_corpus_cond, (None if post is None else C.byref(post), C.byref(cond))
    else:
        fn, extra = (lib.ogg_vorbis_spectral_corpus_sr, ()) if post is None else (lib.ogg_vorbis_spectral_corpus_post, (C.byref(post),))
    res = _corpus.run(lib, fn, list_of_bytes, (threads, feeders, files_per_submit, device, C.byref(spec), target) + extra, (counts,),
                      lambda i, p: _corpus.copy_into(np.zeros((int(counts[i]), dim), np.float32), p), SpectralError, errors, "spectral",
                      stats)
    give_trim_index(trim_index, None, res)
    return _finish(spec, res)


def _finish(spec, res):
    """"stft": each float32 matrix (frames, 2 NB) as its complex64 view (frames, NB); every other kind as it is."""
    if spec.kind == KINDS["stft"]:
        for i, a in enumerate(res):
            if isinstance(a, np.ndarray):
                res[i] = a.view(np.complex64)
    return res


def get_spectral_from_raw_bytes(raw_bytes, kind="log_mel", **kwargs):
    """One file's spectral matrix, shape (frames, dim) float32."""
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return get_spectral_batch([raw_bytes], kind, **kwargs)[0]
