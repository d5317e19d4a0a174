"""Decoded PCM from Ogg bytes, optionally resampled on the GPU: a list of (pcm, sr) like librosa.load. ctypes onto
libparseoggvorbis_amd.so (ogg_vorbis_pcm_corpus). Resampling is scipy.signal.resample_poly with its defaults (librosa's
res_type="polyphase", not its default soxr), computed on the device before the PCM is copied back; the arithmetic is written out
in include/vorbis_synth_hip.h ("resampling") and the float64 model in tests/resample_model.py is the contract.

mono=True returns ONE plane per file, made on the device by the conditioning stage (include/vorbis_synth_hip.h, "PCM
conditioning"; float64 model: tests/condition_model.py): the channels' float32 mean like librosa.load's default, optionally
divided by its peak (peak_normalize) and pre-emphasised (preemphasis), after the resampling and before the copy to the host.
trim_db cuts the silent head and tail of that plane first, as librosa.effects.trim does on a mono signal (include/vorbis_synth_hip.h,
"PCM trimming"; float64 model: tests/trim_model.py). split_db removes every silent stretch instead, as joining the slices of
librosa.effects.split does, and get_intervals_batch returns those intervals alone, without any PCM coming back ("PCM splitting";
model: tests/split_model.py).

Every argument is checked before the library is loaded."""
import ctypes as C
import math

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


COND_PEAK, COND_PREEMPH = 1, 2  # VSYN_COND_PEAK, VSYN_COND_PREEMPH


def cond_spec(peak_normalize=False, preemphasis=None, error=PcmError):
    """Checks the conditioning arguments (include/vorbis_synth_hip.h, "PCM conditioning", step 5) and returns the C spec
    (binding.PcmCond): peak_normalize a bool; preemphasis None or a real number whose float32 rounding lies in (0, 1)."""
    from .binding import PcmCond
    if not isinstance(peak_normalize, (bool, np.bool_)):
        raise error("peak_normalize must be a bool, got %r" % (peak_normalize,))
    opts, a = (COND_PEAK if peak_normalize else 0), 0.0
    if preemphasis is not None:
        if isinstance(preemphasis, (bool, np.bool_)) or not isinstance(preemphasis, (int, float, np.integer, np.floating)):
            raise error("preemphasis must be None or a number in (0, 1), got %r" % (preemphasis,))
        a = float(np.float32(preemphasis))  # rounded once to float32: the coefficient the device uses
        if not (math.isfinite(a) and 0.0 < float(preemphasis) < 1.0 and 0.0 < a < 1.0):
            raise error("preemphasis must be in (0, 1), got %r" % (preemphasis,))
        opts |= COND_PREEMPH
    return PcmCond(opts, 0, a)


TRIM_MAX_FRAME = 8192  # VSYN_TRIM_MAX_FRAME
U32_MAX = 0xFFFFFFFF   # vsyn_pcm_trim's fields are uint32


def trim_spec(trim_db=None, trim_frame_length=2048, trim_hop_length=512, trim_index=None, error=PcmError):
    """Checks the trim arguments (include/vorbis_synth_hip.h, "PCM trimming", step 8) and returns the C spec (binding.PcmTrim), or
    None for trim_db=None: the stage is off and its other arguments are not looked at. trim_db a finite number in (0, 200],
    trim_frame_length an integer in [1, 8192], trim_hop_length an integer >= 1 (that the C spec's uint32 holds), trim_index None
    or a list."""
    from .binding import PcmTrim
    if trim_index is not None and not isinstance(trim_index, list):
        raise error("trim_index must be None or a list, got %r" % (trim_index,))
    if trim_db is None:
        return None
    if isinstance(trim_db, (bool, np.bool_)) or not isinstance(trim_db, (int, float, np.integer, np.floating)):
        raise error("trim_db must be None or a number in (0, 200], got %r" % (trim_db,))
    if not (math.isfinite(float(trim_db)) and 0.0 < float(trim_db) <= 200.0):
        raise error("trim_db must be in (0, 200], got %r" % (trim_db,))
    for name, v, hi in (("trim_frame_length", trim_frame_length, TRIM_MAX_FRAME), ("trim_hop_length", trim_hop_length, U32_MAX)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise error("%s must be an integer, got %r" % (name, v))
        if not 1 <= int(v) <= hi:
            raise error("%s must be in [1, %d], got %d" % (name, hi, int(v)))
    return PcmTrim(int(trim_frame_length), int(trim_hop_length), float(trim_db))


def loudness_args(loudness_normalize, loudness, cond, error=PcmError):
    """Checks the normaliser's arguments (include/vorbis_synth_hip.h, "loudness", steps 6 and 7) and returns the C spec
    (binding.LoudnessSpec: the mono downmix, the target), or None for loudness_normalize=None: the stage is off. loudness None or a
    list; cond: the call's conditioning spec, whose peak normalisation the normaliser excludes."""
    from .loudness import loudness_spec
    if loudness is not None and not isinstance(loudness, list):
        raise error("loudness must be None or a list, got %r" % (loudness,))
    if loudness_normalize is None:
        return None
    spec = loudness_spec("mono", loudness_normalize, lambda msg: error(str(msg).replace("target", "loudness_normalize")))
    if cond.options & COND_PEAK:
        raise error("loudness_normalize and peak_normalize exclude each other: two level controls")
    return spec


def give_loudness(loudness, records, results):
    """loudness[:] = each file's measured LUFS (in front of the gain) from the run's records; None for a failed file, and for every
    file with the stage off (records None)."""
    if loudness is not None:
        from .loudness import lufs_of
        loudness[:] = [None if records is None or isinstance(r, Exception) else float(lufs_of(records[i]["zbar"])) for i, r in enumerate(results)]


def give_trim_index(trim_index, bounds, results):
    """trim_index[:] = one (start, end) per file from the run's bounds array; None for a file that failed, and for every file
    with the stage off (bounds None)."""
    if trim_index is not None:
        trim_index[:] = [None if bounds is None or isinstance(r, Exception) else (int(bounds[i][0]), int(bounds[i][1]))
                         for i, r in enumerate(results)]


def split_spec(split_db=None, split_frame_length=2048, split_hop_length=512, split_index=None, trim=None, error=PcmError):
    """Checks the split arguments as trim_spec checks the trim's (the stage takes the same C spec) and returns it, or None for
    split_db=None: the stage is off. trim: the call's trim spec; a call either trims or splits."""
    if split_index is not None and not isinstance(split_index, list):
        raise error("split_index must be None or a list, got %r" % (split_index,))
    if split_db is None:
        return None

    def renamed(msg):
        return error(str(msg).replace("trim_", "split_"))
    spec = trim_spec(split_db, split_frame_length, split_hop_length, None, renamed)
    if trim is not None:
        raise error("split_db and trim_db exclude each other: the split's first start and last end are the trim's bounds")
    return spec


def give_split_index(split_index, buffers, results):
    """split_index[:] = one (n, 2) int64 array per file from the run's interval buffers; None for a file that failed, and for every
    file with the stage off (buffers None)."""
    if split_index is not None:
        split_index[:] = [None if buffers is None or isinstance(r, Exception) else buffers.take(i) for i, r in enumerate(results)]


def effect_spec(hpss=None, hpss_kernel_size=31, hpss_power=2.0, hpss_margin=1.0, hpss_n_fft=2048, hpss_hop_length=None, hpss_win_length=None,
                error=PcmError):
    """Checks the effect arguments (include/vorbis_synth_hip.h, "PCM effects", step 6) through spectral.hpss_spec and
    spectral.spectral_spec and returns the C spec (binding.PcmEffect), or None for hpss=None: the stage is off and its other
    arguments are not looked at. hpss "harmonic" or "percussive"; hpss_n_fft a power of two in [16, 8192]; hpss_hop_length (None:
    hpss_n_fft // 4) >= 1; hpss_win_length (None: hpss_n_fft) in [1, hpss_n_fft]."""
    if hpss is None:
        return None
    from . import spectral
    from .binding import PcmEffect
    try:
        hp = spectral.hpss_spec(hpss, hpss_kernel_size, hpss_power, hpss_margin, "component")
        n_fft = spectral._int("hpss_n_fft", hpss_n_fft)
        if not (16 <= n_fft <= spectral.MAX_N_FFT and n_fft & (n_fft - 1) == 0):
            raise error("hpss_n_fft must be a power of two in [16, %d], got %d" % (spectral.MAX_N_FFT, n_fft))
        fr = spectral.spectral_spec("stft", n_fft, n_fft // 4 if hpss_hop_length is None else hpss_hop_length, hpss_win_length)
    except spectral.SpectralError as e:
        msg = str(e)  # (spectral_spec names its own arguments: hop_length, win_length)
        raise error(msg if msg.startswith("hpss") else "hpss_" + msg) from None
    return PcmEffect(fr.n_fft, fr.hop_length, fr.win_length, 0, hp)


STRETCH_FIX_LENGTH = 1        # VSYN_STRETCH_FIX_LENGTH
RESAMPLE_MAX_M = 65536        # VSYN_RESAMPLE_MAX_M


def _per_file(name, v, n, error):
    """v, one real number or a sequence of n of them, as a float64 array [n]."""
    if isinstance(v, (bool, np.bool_)):
        raise error("%s must be a number or one number per file, got %r" % (name, v))
    if isinstance(v, (int, float, np.integer, np.floating)):
        return np.full(n, float(v), np.float64)
    try:
        vals = list(v)
    except TypeError:
        raise error("%s must be a number or one number per file, got %r" % (name, v)) from None
    if len(vals) != n:
        raise error("%s has %d values for %d files" % (name, len(vals), n))
    for x in vals:
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise error("%s must hold numbers, got %r" % (name, x))
    return np.array([float(x) for x in vals], np.float64)


def stretch_args(n_files, time_stretch=None, pitch_shift=None, pitch_bins_per_octave=12, stretch_n_fft=2048, stretch_hop_length=None,
                 stretch_win_length=None, sr=None, error=PcmError):
    """Checks the stretch arguments (include/vorbis_synth_hip.h, "PCM stretch", steps 6 and 9) and returns (binding.PcmStretch, rates
    float64 [n_files], shift_from_hz uint32 [n_files] or None), or None with both time_stretch and pitch_shift None: the stage is off
    and its other arguments are not looked at. time_stretch: a finite rate above 0, or one per file (above 1 shortens). pitch_shift:
    finite semitone steps of pitch_bins_per_octave, or one per file; needs sr (an integer: every file at one rate), keeps each
    file's length, and the pair (rint(sr / rate), sr) must be one the resampler takes. The two exclude each other."""
    if time_stretch is None and pitch_shift is None:
        return None
    if time_stretch is not None and pitch_shift is not None:
        raise error("time_stretch and pitch_shift exclude each other in one call")
    from . import spectral
    from .binding import PcmStretch
    try:
        n_fft = spectral._int("stretch_n_fft", stretch_n_fft)
        if not (16 <= n_fft <= spectral.MAX_N_FFT and n_fft & (n_fft - 1) == 0):
            raise error("stretch_n_fft must be a power of two in [16, %d], got %d" % (spectral.MAX_N_FFT, n_fft))
        fr = spectral.spectral_spec("stft", n_fft, n_fft // 4 if stretch_hop_length is None else stretch_hop_length, stretch_win_length)
    except spectral.SpectralError as e:
        msg = str(e)  # (spectral_spec names its own arguments: hop_length, win_length)
        raise error(msg if msg.startswith("stretch") else "stretch_" + msg) from None
    if time_stretch is not None:
        rates = _per_file("time_stretch", time_stretch, n_files, error)
        for r in rates:
            if not (math.isfinite(r) and r > 0.0):
                raise error("time_stretch must be a finite rate above 0, got %r" % (float(r),))
        return PcmStretch(fr.n_fft, fr.hop_length, fr.win_length, 0, 0, 0), rates, None
    steps = _per_file("pitch_shift", pitch_shift, n_files, error)
    if isinstance(pitch_bins_per_octave, (bool, np.bool_)) or not isinstance(pitch_bins_per_octave, (int, np.integer)) or pitch_bins_per_octave < 1:
        raise error("pitch_bins_per_octave must be an integer >= 1, got %r" % (pitch_bins_per_octave,))
    if sr is None:
        raise error("pitch_shift needs sr=: every file is resampled to one rate first, and back to it behind the stretch")
    rates, from_hz = np.zeros(n_files, np.float64), np.zeros(n_files, np.uint32)
    for i, st in enumerate(steps):
        r = 2.0 ** (-float(st) / int(pitch_bins_per_octave)) if math.isfinite(st) else float("nan")
        if not (math.isfinite(r) and r > 0.0):
            raise error("pitch_shift must be a finite number of steps whose rate 2^(-steps / bins) is a finite rate above 0, got %r" % (float(st),))
        hz = float(np.rint(int(sr) / r))
        if not 1.0 <= hz <= MAX_RATE:
            raise error("pitch_shift %r: the rate %g Hz to resample from is outside [1, %d]" % (float(st), hz, MAX_RATE))
        g = math.gcd(int(hz), int(sr))
        if max(int(hz), int(sr)) // g > RESAMPLE_MAX_M:
            raise error("pitch_shift %r: resample: %d -> %d Hz reduces to %d / %d, above the limit max(up, down) <= %d"
                        % (float(st), int(hz), int(sr), int(sr) // g, int(hz) // g, RESAMPLE_MAX_M))
        rates[i], from_hz[i] = r, int(hz)
    return PcmStretch(fr.n_fft, fr.hop_length, fr.win_length, STRETCH_FIX_LENGTH, int(sr), 0), rates, from_hz


_load = _corpus.load


def get_pcm_batch(list_of_bytes, sr=None, dtype="float32", threads=0, feeders=0, device=0, errors="raise", files_per_submit=64,
                  stats=None, mono=False, peak_normalize=False, preemphasis=None, trim_db=None, trim_frame_length=2048, trim_hop_length=512,
                  trim_index=None, split_db=None, split_frame_length=2048, split_hop_length=512, split_index=None, loudness_normalize=None,
                  loudness=None, hpss=None, hpss_kernel_size=31, hpss_power=2.0, hpss_margin=1.0, hpss_n_fft=2048, hpss_hop_length=None,
                  hpss_win_length=None, time_stretch=None, pitch_shift=None, pitch_bins_per_octave=12, stretch_n_fft=2048, stretch_hop_length=None,
                  stretch_win_length=None):
    """PCM of many Ogg Vorbis files in one corpus run: a list of (pcm, sr) tuples. pcm is float32 (channels, frames), or int16
    (frames, channels) with ov_read's conversion; sr is the rate of the returned PCM. sr=None keeps each file's own rate (the
    PCM is bit for bit that of ogg_vorbis_decode_corpus); an integer resamples every file to it on the GPU. errors="raise": the
    first failed file raises PcmError naming it; errors="return": its entry is the PcmError. stats (optional list) receives
    the run's 8 corpus statistics.
    mono=True: pcm is 1-D (frames,), float32 or int16, the channels' mean computed on the device (half the bytes come back for
    stereo files); with peak_normalize=True divided by its largest magnitude, so that the peak is exactly +-1 (a file with an Inf
    or NaN sample fails alone; silence stays silence); with preemphasis=a, 0 < a < 1, then filtered as z[t] = y[t] - a y[t-1].
    peak_normalize and preemphasis need mono=True.
    trim_db=d (0 < d <= 200, needs mono=True): the leading and trailing frames of the mono signal whose RMS over trim_frame_length
    samples, every trim_hop_length samples, lies more than d dB below the loudest frame's are cut off first, as
    librosa.effects.trim(y, top_db=d) does; the peak and the pre-emphasis are those of what is kept. trim_index (optional list)
    receives one (start, end) per file, in samples of the returned rate (None for a failed file, and for every file with the stage off). A
    file with an Inf or NaN sample fails alone.
    split_db=d (instead of trim_db, with split_frame_length and split_hop_length; needs mono=True): every stretch of such frames is
    removed, not the head and the tail alone: pcm is the concatenation of y[start:end] over librosa.effects.split(y, top_db=d)'s
    intervals, and the peak and the pre-emphasis are those of that joined signal. split_index (optional list) receives one (n, 2)
    int64 array of (start, end) per file (None for a failed file, and for every file with the stage off).
    loudness_normalize=L (a number of LUFS in [-70, 0]; needs mono=True, excludes peak_normalize): the mono signal, behind the
    resampler and trim_db / split_db and in front of the pre-emphasis, is scaled by one gain so that its integrated loudness (ITU-R
    BS.1770-4, as get_loudness_batch(channels="mono") measures it on that signal) is L; it is not clipped. loudness (optional list)
    receives the measured LUFS per file, in front of the gain (None for a failed file, and for every file with the stage off). A
    file that is shorter than 400 ms, silent (nothing above -70 LUFS), not finite or below 4000 Hz fails alone, by name. With
    loudness_normalize=None nothing is launched and the call takes the entry points it took without the argument.
    hpss="harmonic" or "percussive" (needs mono=True): the mono signal, behind the resampler and trim_db / split_db and in front of
    the loudness normaliser, the peak and the pre-emphasis, is replaced by that component of it, as librosa.effects.harmonic(y,
    kernel_size=hpss_kernel_size, power=hpss_power, margin=hpss_margin, n_fft=hpss_n_fft, hop_length=hpss_hop_length,
    win_length=hpss_win_length) computes it (percussive likewise): STFT, the soft mask of decompose.hpss on its magnitude, the masked
    inverse STFT to the signal's own length, all on the device. hpss_n_fft is a power of two in [16, 8192]; hpss_hop_length defaults
    to hpss_n_fft // 4 and hpss_win_length to hpss_n_fft; hpss_kernel_size and hpss_margin are one value or a (harmonic, percussive)
    pair. With hpss=None nothing is launched and the call takes the entry points it took without the argument.
    time_stretch=r (a finite rate above 0, or one per file; needs mono=True, excludes hpss): in the same place the mono signal is
    time-stretched as librosa.effects.time_stretch(y, rate=r, n_fft=stretch_n_fft, hop_length=stretch_hop_length,
    win_length=stretch_win_length) does: STFT, phase vocoder, inverse STFT to round(len(y) / r) samples, all on the device. r above 1
    shortens. pitch_shift=s (semitone steps of pitch_bins_per_octave, or one per file; needs mono=True and sr=, excludes
    time_stretch and hpss) shifts the pitch and keeps the length, as librosa.effects.pitch_shift(y, sr=sr, n_steps=s,
    bins_per_octave=pitch_bins_per_octave) does: the stretch at rate 2^(-s / bins), then resampled from rint(sr / rate) Hz back to sr
    and cut or zero-padded to len(y). librosa resamples from the unrounded sr / rate; the whole-Hz rate moves the pitch by at most
    0.5 / (sr / rate) relative. A pair of rates the resampler refuses raises by name before anything runs. With both None nothing is
    launched and the call takes the entry points it took without the arguments."""
    _corpus.check_errors(errors)
    target = check_sr(sr)
    name = _format(dtype)
    if not isinstance(mono, (bool, np.bool_)):
        raise PcmError("mono must be a bool, got %r" % (mono,))
    cond = cond_spec(peak_normalize, preemphasis)
    if not mono and cond.options:
        raise PcmError("peak_normalize and preemphasis act on the mono signal: pass mono=True")
    trim = trim_spec(trim_db, trim_frame_length, trim_hop_length, trim_index)
    if not mono and trim is not None:
        raise PcmError("trim_db acts on the mono signal: pass mono=True")
    split = split_spec(split_db, split_frame_length, split_hop_length, split_index, trim)
    if not mono and split is not None:
        raise PcmError("split_db acts on the mono signal: pass mono=True")
    loud = loudness_args(loudness_normalize, loudness, cond)
    if not mono and loud is not None:
        raise PcmError("loudness_normalize acts on the mono signal: pass mono=True")
    effect = effect_spec(hpss, hpss_kernel_size, hpss_power, hpss_margin, hpss_n_fft, hpss_hop_length, hpss_win_length)
    if not mono and effect is not None:
        raise PcmError("hpss acts on the mono signal: pass mono=True")
    n = len(list_of_bytes)
    stretch = stretch_args(n, time_stretch, pitch_shift, pitch_bins_per_octave, stretch_n_fft, stretch_hop_length, stretch_win_length, sr)
    if stretch is not None and not mono:
        raise PcmError("time_stretch and pitch_shift act on the mono signal: pass mono=True")
    if stretch is not None and effect is not None:
        raise PcmError("time_stretch / pitch_shift and hpss exclude each other: their composition is not built")
    lib = _load()
    frames = np.zeros(n, np.uint64)
    chans = np.zeros(n, np.uint32)
    rates = np.zeros(n, np.uint32)

    def build(i, p):
        T, Cn = int(frames[i]), int(chans[i])
        if mono:
            a = np.zeros(T, np.float32 if name == "float32" else np.int16)
        else:
            a = np.zeros((Cn, T), np.float32) if name == "float32" else np.zeros((T, Cn), np.int16)
        return _corpus.copy_into(a, p), int(rates[i])

    args = (threads, feeders, files_per_submit, device, target, FORMATS[name])
    if loud is not None or effect is not None or stretch is not None:  # the entries with every stage's spec (NULL: off); the effect and the stretch have their own
        from .binding import LOUDNESS_RECORD_DTYPE
        ib = _corpus.IntervalBuffers(lib, n)
        bounds, records = np.zeros((max(n, 1), 2), np.uint64), np.zeros(max(n, 1), LOUDNESS_RECORD_DTYPE)
        gate = split if split is not None else trim
        head = (C.byref(cond) if cond.options else None, None if gate is None else C.byref(gate), int(split is not None))
        if stretch is not None:
            st_spec, st_rates, st_from = stretch
            fn, specs = lib.ogg_vorbis_pcm_corpus_stretch, (None, C.byref(st_spec), st_rates.ctypes.data,
                                                            None if st_from is None else st_from.ctypes.data,
                                                            None if loud is None else C.byref(loud))
        elif effect is None:
            fn, specs = lib.ogg_vorbis_pcm_corpus_loud, (C.byref(loud),)
        else:
            fn, specs = lib.ogg_vorbis_pcm_corpus_effects, (C.byref(effect), None if loud is None else C.byref(loud))
        try:
            res = _corpus.run(lib, fn, list_of_bytes, args + head + specs, (frames, chans, rates, bounds, ib.ptrs, ib.counts, records), build,
                              PcmError, errors, "pcm", stats)
            give_split_index(split_index, ib if split is not None else None, res)
        finally:
            ib.free()
        give_trim_index(trim_index, bounds[:n] if trim is not None else None, res)
        give_loudness(loudness, records if loud is not None else None, res)
        return res
    give_loudness(loudness, None, [None] * n)
    if split is not None:
        ib = _corpus.IntervalBuffers(lib, n)
        try:
            res = _corpus.run(lib, lib.ogg_vorbis_pcm_corpus_split, list_of_bytes, args + (C.byref(cond) if cond.options else None, C.byref(split)),
                              (frames, chans, rates, ib.ptrs, ib.counts), build, PcmError, errors, "pcm", stats)
            give_split_index(split_index, ib, res)
        finally:
            ib.free()
        give_trim_index(trim_index, None, res)
        return res
    give_split_index(split_index, None, [None] * n)
    if trim is not None:
        bounds = np.zeros((max(n, 1), 2), np.uint64)
        res = _corpus.run(lib, lib.ogg_vorbis_pcm_corpus_trim, list_of_bytes, args + (C.byref(cond) if cond.options else None, C.byref(trim)),
                          (frames, chans, rates, bounds), build, PcmError, errors, "pcm", stats)
        give_trim_index(trim_index, bounds[:n], res)
        return res
    fn, extra = (lib.ogg_vorbis_pcm_corpus_cond, (C.byref(cond),)) if mono else (lib.ogg_vorbis_pcm_corpus, ())
    res = _corpus.run(lib, fn, list_of_bytes, args + extra, (frames, chans, rates), build, PcmError, errors, "pcm", stats)
    give_trim_index(trim_index, None, res)
    return res


def get_intervals_batch(list_of_bytes, top_db=60.0, frame_length=2048, hop_length=512, sr=None, threads=0, feeders=0, device=0, errors="raise",
                        files_per_submit=64, stats=None):
    """The non-silent intervals of many Ogg Vorbis files in one corpus run: a list of (intervals, sr, frames) tuples. intervals is
    an (n, 2) int64 array of (start, end) in samples, what librosa.effects.split(y, top_db=top_db, frame_length=frame_length,
    hop_length=hop_length) returns for the mono signal y = get_pcm_batch(mono=True, sr=sr); sr is the rate they are counted at and
    frames the length of y. The frame energies and the intervals are computed on the device and no PCM is copied back. sr, errors
    and stats as for get_pcm_batch; a file with an Inf or NaN sample fails alone."""
    _corpus.check_errors(errors)
    target = check_sr(sr)

    def renamed(msg):
        return PcmError(str(msg).replace("trim_db", "top_db").replace("trim_", ""))
    if top_db is None:
        raise PcmError("top_db must be a number in (0, 200], got None")
    split = trim_spec(top_db, frame_length, hop_length, None, renamed)
    lib = _load()
    n = len(list_of_bytes)
    counts = np.zeros(max(n, 1), np.uint64)
    frames = np.zeros(max(n, 1), np.uint64)
    rates = np.zeros(max(n, 1), np.uint32)

    def build(i, p):
        return _corpus.copy_into(np.zeros((int(counts[i]), 2), np.uint32), p).astype(np.int64), int(rates[i]), int(frames[i])

    return _corpus.run(lib, lib.ogg_vorbis_intervals_corpus, list_of_bytes, (threads, feeders, files_per_submit, device, target, C.byref(split)),
                       (counts, frames, rates), build, PcmError, errors, "intervals", stats)


def get_intervals_from_raw_bytes(raw_bytes, top_db=60.0, **kwargs):
    """One file's (intervals, sr, frames), as get_intervals_batch."""
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return get_intervals_batch([raw_bytes], top_db, **kwargs)[0]


def get_pcm_from_raw_bytes(raw_bytes, sr=None, dtype="float32", **kwargs):
    """One file's (pcm, sr), as get_pcm_batch."""
    kwargs.setdefault("threads", 1)
    kwargs.setdefault("feeders", 1)
    return get_pcm_batch([raw_bytes], sr, dtype, **kwargs)[0]
