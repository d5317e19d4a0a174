"""Rhythm features of Ogg Vorbis files on the GPU: onset strength, onset frames, tempogram, tempo and beats (include/vorbis_synth_hip.h,
"rhythm"; models: tests/rhythm_model.py, tests/beat_model.py). The spectral rows never leave the device: the onset stage reads them where the spectral
kernels (and HPSS, PCEN) left them, and only the selected output comes back.

Every entry forwards the arguments of spectral.get_spectral_batch that shape the rows or the PCM in front of them (kind and the STFT /
mel arguments, sr, trim_* / split_*, loudness_normalize, peak_normalize / preemphasis, hpss*, pcen*, threads, feeders, device, errors,
files_per_submit, stats) as keywords, checked by the same code (spectral.checked_specs); kind defaults to "mel_db", which is what
librosa.onset.onset_strength(y, sr) feeds itself. delta / normalize are refused by name (the onset stage takes their place), and so is
a kind whose rows are wider than 256 columns. Every argument is checked before the library loads."""
import ctypes as C
import inspect
import math

import numpy as np

from . import _corpus
from .spectral import CHROMA_KINDS, SpectralError, checked_specs, get_spectral_batch

MAX_DIM = 256
MAX_LAG = 64
MAX_WIN_LENGTH = 2048
OUTPUTS = {"envelope": 0, "onsets": 1, "tempogram": 2, "tempo_mean": 3}
_REFUSED = ("delta", "delta_width", "normalize", "std_floor")
_DEFAULTS = {k: p.default for k, p in inspect.signature(get_spectral_batch).parameters.items() if p.default is not inspect.Parameter.empty}


class RhythmError(SpectralError):
    pass


def _int(name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise RhythmError("%s must be an integer in [%d, %d], got %r" % (name, lo, hi, v))
    return int(v)


def _number(name, v, lo=None, positive=False):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
        raise RhythmError("%s must be a finite number, got %r" % (name, v))
    v = float(v)
    if (lo is not None and v < lo) or (positive and not v > 0.0):
        raise RhythmError("%s must be %s, got %r" % (name, "> 0" if positive else ">= %g" % lo, v))
    return v


def _flag(name, v):
    if not isinstance(v, (bool, np.bool_)):
        raise RhythmError("%s must be True or False, got %r" % (name, v))
    return bool(v)


def onset_spec(lag=1, max_size=1, n_fft=2048, hop_length=512, center=True):
    """binding.OnsetSpec of checked arguments: lag and max_size in [1, 64]."""
    from .binding import OnsetSpec
    return OnsetSpec(_int("lag", lag, 1, MAX_LAG), _int("max_size", max_size, 1, 64), _int("n_fft", n_fft, 1, 2 ** 31 - 1),
                     _int("hop_length", hop_length, 1, 2 ** 31 - 1), 1 if _flag("center", center) else 0)


def peaks_spec(pre_max=0.03, post_max=0.0, pre_avg=0.10, post_avg=0.10, wait=0.03, delta=0.07, normalize=True, hop_length=512):
    """binding.OnsetPeaks of checked arguments: the five times in seconds, finite and >= 0; delta finite."""
    from .binding import OnsetPeaks
    t = [_number(n, v, lo=0.0) for n, v in (("pre_max", pre_max), ("post_max", post_max), ("pre_avg", pre_avg), ("post_avg", post_avg), ("wait", wait))]
    return OnsetPeaks(t[0], t[1], t[2], t[3], t[4], _number("delta", delta), _int("hop_length", hop_length, 1, 2 ** 31 - 1),
                      1 if _flag("normalize", normalize) else 0)


def tempogram_spec(win_length=384, tg_center=True, norm=math.inf, hop_length=512, ac_size=None):
    """binding.TempogramSpec of checked arguments: win_length in [2, 2048], or None with ac_size (seconds) for a window length from
    each file's rate; norm numpy.inf or None."""
    from .binding import TempogramSpec
    if norm is not None and not (isinstance(norm, (float, np.floating)) and norm == math.inf):
        raise RhythmError("norm must be numpy.inf or None, got %r" % (norm,))
    if (win_length is None) == (ac_size is None):
        raise RhythmError("one of win_length and ac_size must be given")
    w = 0 if win_length is None else _int("win_length", win_length, 2, MAX_WIN_LENGTH)
    return TempogramSpec(w, _int("hop_length", hop_length, 1, 2 ** 31 - 1), (1 if _flag("tg_center", tg_center) else 0) | (0 if norm is None else 2), 0,
                         0.0 if ac_size is None else _number("ac_size", ac_size, positive=True))


def tempo_spec(start_bpm=120.0, std_bpm=1.0, max_tempo=320.0):
    """binding.TempoSpec of checked arguments; max_tempo None: no cap."""
    from .binding import TempoSpec
    return TempoSpec(_number("start_bpm", start_bpm, positive=True), _number("std_bpm", std_bpm, positive=True),
                     0.0 if max_tempo is None else _number("max_tempo", max_tempo, positive=True))


def beat_spec(tightness=100.0, start_bpm=120.0, bpm=None, trim=True, hop_length=512):
    """binding.BeatSpec of checked arguments: tightness and start_bpm finite and > 0; bpm None (estimated per file) or finite and > 0."""
    from .binding import BeatSpec
    return BeatSpec(_number("tightness", tightness, positive=True), _number("start_bpm", start_bpm, positive=True),
                    0.0 if bpm is None else _number("bpm", bpm, positive=True), _int("hop_length", hop_length, 1, 2 ** 31 - 1),
                    1 if _flag("trim", trim) else 0)


def _spectral_args(kw):
    """The forwarded get_spectral_batch arguments, every one checked: (checked_specs' result, the merged dict)."""
    for k in kw:
        if k in _REFUSED:
            raise RhythmError("%s is not available with the rhythm stages: the onset stage takes the place of delta / normalize" % k)
        if k not in _DEFAULTS:
            raise RhythmError("unknown argument %r" % k)
    a = dict(_DEFAULTS, kind="mel_db")
    a.update(kw)
    try:
        c = checked_specs(a)
    except RhythmError:
        raise
    except SpectralError as e:
        raise RhythmError(str(e)) from None
    if a["kind"] == "stft" or c.dim > MAX_DIM:
        raise RhythmError("kind %r is not available with the rhythm stages: its rows have %d columns, the onset stage holds %d"
                          % (a["kind"], c.dim, MAX_DIM))
    return c, a


def _run(list_of_bytes, rhythm, build, c, a):
    """One corpus run through ogg_vorbis_rhythm_corpus: per file build(words, rows) of the selected output, or the RhythmError."""
    from .binding import LOUDNESS_RECORD_DTYPE
    from .pcm import give_loudness, give_split_index, give_trim_index
    lib = _corpus.load()
    n = len(list_of_bytes)
    counts = np.zeros(max(n, 1), np.uint64)
    ib = _corpus.IntervalBuffers(lib, n)
    joined, bounds = np.zeros(max(n, 1), np.uint64), np.zeros((max(n, 1), 2), np.uint64)
    records = np.zeros(max(n, 1), LOUDNESS_RECORD_DTYPE)
    gate = c.split if c.split is not None else c.trim
    cols = {0: 1, 1: 1, 2: rhythm.tempogram.win_length, 3: 2}[rhythm.output]
    try:
        res = _corpus.run(lib, lib.ogg_vorbis_rhythm_corpus, list_of_bytes,
                          (a["threads"], a["feeders"], a["files_per_submit"], a["device"], C.byref(c.spec),
                           C.byref(c.chroma) if a["kind"] in CHROMA_KINDS else None, c.target,
                           C.byref(c.hp) if a["hpss"] is not None else None, C.byref(c.pc) if a["pcen"] else None, None, C.byref(rhythm),
                           C.byref(c.cond) if c.cond.options else None, None if gate is None else C.byref(gate), int(c.split is not None),
                           None if c.loud is None else C.byref(c.loud)),
                          (counts, bounds, joined, ib.ptrs, ib.counts, records),
                          lambda i, p: build(_corpus.copy_into(np.zeros(int(counts[i]) * cols, np.uint32), p), int(counts[i])), RhythmError,
                          a["errors"], "rhythm", a["stats"])
        give_split_index(a["split_index"], ib if c.split is not None else None, res)
    finally:
        ib.free()
    give_trim_index(a["trim_index"], bounds[:n] if c.trim is not None else None, res)
    give_loudness(a["loudness"], records if c.loud is not None else None, res)
    return res


def _rhythm_spec(output, c, lag, max_size, peaks=None, tempogram=None):
    from .binding import RhythmSpec
    hop, n_fft, center = c.spec.hop_length, c.spec.n_fft, bool(c.spec.options & 1)
    r = RhythmSpec()
    r.output = OUTPUTS[output]
    r.onset = onset_spec(lag, max_size, n_fft, hop, center)
    if peaks is not None:
        r.peaks = peaks_spec(hop_length=hop, **peaks)
    if tempogram is not None:
        r.tempogram = tempogram_spec(hop_length=hop, **tempogram)
    return r


def get_onset_strength_batch(list_of_bytes, lag=1, max_size=1, **spectral):
    """librosa.onset.onset_strength(S=rows.T, lag=lag, max_size=max_size, aggregate=numpy.mean) of every file's rows (kind "mel_db" by
    default; center is the spectral argument): a list of float32 arrays (frames,), exactly as many entries as the rows."""
    c, a = _spectral_args(spectral)
    r = _rhythm_spec("envelope", c, lag, max_size)
    return _run(list_of_bytes, r, lambda w, rows: w.view(np.float32), c, a)


def get_onsets_batch(list_of_bytes, lag=1, max_size=1, pre_max=0.03, post_max=0.0, pre_avg=0.10, post_avg=0.10, wait=0.03, delta=0.07,
                     normalize=True, envelope=None, **spectral):
    """librosa.onset.onset_detect(onset_envelope=that envelope, backtrack=False, units="frames") with util.peak_pick's clipped windows:
    a list of int64 frame arrays. The times are seconds, turned into frames at each file's rate. A file whose envelope holds an Inf or
    a NaN fails alone. envelope (optional list) receives each file's envelope (None for a failed file), from a second run of the same
    arithmetic."""
    c, a = _spectral_args(spectral)
    pk = dict(pre_max=pre_max, post_max=post_max, pre_avg=pre_avg, post_avg=post_avg, wait=wait, delta=delta, normalize=normalize)
    r = _rhythm_spec("onsets", c, lag, max_size, peaks=pk)
    if envelope is not None and not isinstance(envelope, list):
        raise RhythmError("envelope must be a list or None")
    res = _run(list_of_bytes, r, lambda w, rows: w.astype(np.int64), c, a)
    if envelope is not None:
        quiet = dict(spectral, errors="return", stats=None, trim_index=None, split_index=None, loudness=None)
        env = get_onset_strength_batch(list_of_bytes, lag, max_size, **quiet)
        envelope[:] = [e if isinstance(e, np.ndarray) and isinstance(o, np.ndarray) else None for e, o in zip(env, res)]
    return res


def get_tempogram_batch(list_of_bytes, lag=1, max_size=1, win_length=384, tg_center=True, norm=math.inf, **spectral):
    """librosa.feature.tempogram(onset_envelope=that envelope, win_length=win_length, center=tg_center, window="hann", norm=norm): a
    list of float32 arrays (frames', win_length), time-major; frames' = frames with tg_center, else max(0, frames - win_length + 1)."""
    c, a = _spectral_args(spectral)
    if win_length is None:
        raise RhythmError("win_length must be an integer in [2, %d]" % MAX_WIN_LENGTH)
    r = _rhythm_spec("tempogram", c, lag, max_size, tempogram=dict(win_length=win_length, tg_center=tg_center, norm=norm))
    W = r.tempogram.win_length
    return _run(list_of_bytes, r, lambda w, rows: w.view(np.float32).reshape(rows, W), c, a)


def get_tempo_batch(list_of_bytes, lag=1, max_size=1, ac_size=8.0, start_bpm=120.0, std_bpm=1.0, max_tempo=320.0, tempogram_mean=None,
                    **spectral):
    """librosa.feature.tempo(onset_envelope=that envelope, sr=sr, hop_length=hop_length, ac_size=ac_size, start_bpm=start_bpm,
    std_bpm=std_bpm, max_tempo=max_tempo, aggregate=numpy.mean): a list of (bpm, sr), sr the rate the rows were computed at. Only the
    mean tempogram, floor(ac_size sr / hop_length) float64 values a file, leaves the device; the prior and the arg-max are the library's
    host arithmetic. A file whose window length falls outside [2, 2048], or whose mean is not finite (no frames, for one), fails alone.
    tempogram_mean (optional list) receives each file's mean (None for a failed file)."""
    from . import binding
    c, a = _spectral_args(spectral)
    ts = tempo_spec(start_bpm, std_bpm, max_tempo)
    if tempogram_mean is not None and not isinstance(tempogram_mean, list):
        raise RhythmError("tempogram_mean must be a list or None")
    r = _rhythm_spec("tempo_mean", c, lag, max_size, tempogram=dict(win_length=None, ac_size=ac_size, tg_center=True, norm=math.inf))
    hop = c.spec.hop_length
    errors = a["errors"]
    res = _run(list_of_bytes, r, lambda w, rows: w.view(np.float64), c, dict(a, errors="return"))
    out, means = [], []
    for i, m in enumerate(res):
        e = m
        if isinstance(m, np.ndarray):
            if len(m) < 3:
                e = RhythmError("file %d: rhythm: no frames to take a tempo from" % i)
            else:
                try:
                    e = (binding.tempo_from_mean(ts, m[:-1], int(m[-1]), hop)[0], int(m[-1]))
                except binding.VsynError as ve:
                    e = RhythmError("file %d: rhythm: %s" % (i, ve))
        if isinstance(e, Exception) and errors == "raise":
            raise e
        out.append(e)
        means.append(m[:-1].copy() if isinstance(e, tuple) else None)
    if tempogram_mean is not None:
        tempogram_mean[:] = means
    return out


def _run_beats(list_of_bytes, onset, beat, c, a):
    """One corpus run through ogg_vorbis_beats_corpus: per file (bpm, beats int64, sr), or the RhythmError."""
    from .binding import LOUDNESS_RECORD_DTYPE
    from .pcm import give_loudness, give_split_index, give_trim_index
    lib = _corpus.load()
    n = len(list_of_bytes)
    counts = np.zeros(max(n, 1), np.uint64)
    bpm, rate = np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.uint32)
    ib = _corpus.IntervalBuffers(lib, n)
    joined, bounds = np.zeros(max(n, 1), np.uint64), np.zeros((max(n, 1), 2), np.uint64)
    records = np.zeros(max(n, 1), LOUDNESS_RECORD_DTYPE)
    gate = c.split if c.split is not None else c.trim
    try:
        res = _corpus.run(lib, lib.ogg_vorbis_beats_corpus, list_of_bytes,
                          (a["threads"], a["feeders"], a["files_per_submit"], a["device"], C.byref(c.spec),
                           C.byref(c.chroma) if a["kind"] in CHROMA_KINDS else None, c.target,
                           C.byref(c.hp) if a["hpss"] is not None else None, C.byref(c.pc) if a["pcen"] else None, None, C.byref(onset),
                           C.byref(beat), C.byref(c.cond) if c.cond.options else None, None if gate is None else C.byref(gate),
                           int(c.split is not None), None if c.loud is None else C.byref(c.loud)),
                          (counts, bpm, rate, bounds, joined, ib.ptrs, ib.counts, records),
                          lambda i, p: (float(bpm[i]), _corpus.copy_into(np.zeros(int(counts[i]), np.uint32), p).astype(np.int64), int(rate[i])),
                          RhythmError, a["errors"], "beats", a["stats"])
        give_split_index(a["split_index"], ib if c.split is not None else None, res)
    finally:
        ib.free()
    give_trim_index(a["trim_index"], bounds[:n] if c.trim is not None else None, res)
    give_loudness(a["loudness"], records if c.loud is not None else None, res)
    return res


def get_beats_batch(list_of_bytes, lag=1, max_size=1, start_bpm=120.0, tightness=100.0, trim=True, bpm=None, envelope=None, **spectral):
    """librosa.beat.beat_track(onset_envelope=that envelope, sr=sr, hop_length=hop_length, start_bpm=start_bpm, tightness=tightness,
    trim=trim, bpm=bpm, units="frames") with the envelope of get_onset_strength_batch (its mean aggregate): a list of (bpm, beats
    int64, sr), sr the rate the rows were computed at. bpm None: each file's own tempo, as get_tempo_batch(ac_size=8.0) gives it; a
    number: that tempo for every file; a list: one entry per file (files of one tempo share a run). A file without beats to take a
    tempo from (fewer than two frames, an all-zero envelope) returns (0.0, no beats, sr). A file whose envelope is not finite, whose
    tempo window length falls outside [2, 2048] or whose beat period falls outside [1, 2048] frames fails alone. envelope (optional
    list) receives each file's envelope (None for a failed file), from a second run of the same arithmetic."""
    c, a = _spectral_args(spectral)
    hop, n_fft, center = c.spec.hop_length, c.spec.n_fft, bool(c.spec.options & 1)
    onset = onset_spec(lag, max_size, n_fft, hop, center)
    n = len(list_of_bytes)
    if isinstance(bpm, (list, tuple, np.ndarray)):
        if len(bpm) != n:
            raise RhythmError("bpm must be a number, None or a list with one entry per file, got %d entries for %d files" % (len(bpm), n))
        per_file = [_number("bpm", v, positive=True) for v in bpm]
    else:
        per_file = [None if bpm is None else _number("bpm", bpm, positive=True)] * n
    specs = {v: beat_spec(tightness, start_bpm, v, trim, hop) for v in set(per_file)} or {None: beat_spec(tightness, start_bpm, None, trim, hop)}
    if envelope is not None and not isinstance(envelope, list):
        raise RhythmError("envelope must be a list or None")
    _corpus.check_errors(a["errors"])
    if len(specs) == 1:
        res = _run_beats(list_of_bytes, onset, next(iter(specs.values())), c, a)
    else:  # one run per tempo, each over its files; the per-file side outputs are not split across runs
        if a["trim_index"] is not None or a["split_index"] is not None or a["loudness"] is not None or a["stats"] is not None:
            raise RhythmError("trim_index, split_index, loudness and stats are not available with a list of bpm")
        res = [None] * n
        for v, bs in specs.items():
            idx = [i for i in range(n) if per_file[i] == v]
            part = _run_beats([list_of_bytes[i] for i in idx], onset, bs, c, dict(a, errors="return"))
            for i, r in zip(idx, part):
                res[i] = RhythmError(str(r).replace("file %d:" % idx.index(i), "file %d:" % i, 1)) if isinstance(r, Exception) else r
        if a["errors"] == "raise":
            for r in res:
                if isinstance(r, Exception):
                    raise r
    if envelope is not None:
        quiet = dict(spectral, errors="return", stats=None, trim_index=None, split_index=None, loudness=None)
        env = get_onset_strength_batch(list_of_bytes, lag, max_size, **quiet)
        envelope[:] = [e if isinstance(e, np.ndarray) and isinstance(o, tuple) else None for e, o in zip(env, res)]
    return res


def _single(fn, raw_bytes, kwargs):
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return fn([raw_bytes], **kwargs)[0]


def get_onset_strength_from_raw_bytes(raw_bytes, **kwargs):
    """One file's onset strength envelope, float32 (frames,)."""
    return _single(get_onset_strength_batch, raw_bytes, kwargs)


def get_onsets_from_raw_bytes(raw_bytes, **kwargs):
    """One file's onset frames, int64."""
    return _single(get_onsets_batch, raw_bytes, kwargs)


def get_tempogram_from_raw_bytes(raw_bytes, **kwargs):
    """One file's tempogram, float32 (frames', win_length)."""
    return _single(get_tempogram_batch, raw_bytes, kwargs)


def get_beats_from_raw_bytes(raw_bytes, **kwargs):
    """One file's (bpm, beats int64, sr)."""
    return _single(get_beats_batch, raw_bytes, kwargs)


def get_tempo_from_raw_bytes(raw_bytes, **kwargs):
    """One file's (bpm, sr)."""
    return _single(get_tempo_batch, raw_bytes, kwargs)
