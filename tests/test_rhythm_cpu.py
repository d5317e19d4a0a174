"""The rhythm model (tests/rhythm_model.py) against restatements in numpy's and scipy's own words, the host-side arithmetic of the
library (window lengths, the tempogram's tile, the tempo) against the model, and the decidedness of every test input. No GPU."""
import ctypes as C

import numpy as np
import pytest
import scipy.ndimage
import scipy.signal

import __graft_entry__ as entry
from parseoggvorbis_amd import binding
from tests import rhythm_cases as rc
from tests import rhythm_model as rm


@pytest.fixture(scope="module")
def lib():
    entry.build_hip()
    return binding.load()


# ---- onset strength -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 8, 9, 20, 64])
@pytest.mark.parametrize("D", [1, 2, 7, 40])
def test_reference_rows_are_scipys_maximum_filter(D, m):
    """Even sizes (not centred) and sizes above D (the reflection repeats)."""
    S = rm.rows(9, D, 10 * D + m)
    assert np.array_equal(rm.ref_rows(S, m), scipy.ndimage.maximum_filter1d(S, m, axis=1, mode="reflect"))


def test_reference_rows_hand_a_nan_on():
    S = rm.rows(3, 12, 1)
    S[1, 5] = np.nan
    S[2, 0] = np.inf
    R = rm.ref_rows(S, 4)  # window of j: [j - 2, j + 2)
    assert np.array_equal(np.isnan(R[1]), [4 <= j <= 7 for j in range(12)])
    assert np.all(np.isinf(R[2, :3])) and np.isfinite(R[2, 3:]).all() and np.isfinite(R[0]).all()  # (bin 0 is also bin -1's mirror)


@pytest.mark.parametrize("lag,max_size,center,n_fft,hop", [(1, 1, True, 2048, 512), (2, 3, True, 2048, 512), (5, 8, False, 2048, 512),
                                                        (1, 1, True, 1024, 73), (64, 64, True, 400, 160)])
def test_envelope_in_numpys_words(lag, max_size, center, n_fft, hop):
    """librosa.onset.onset_strength_multi with aggregate = mean: ref = maximum_filter1d(S); onset_env = S[lag:] - ref[:-lag];
    maximum(0, .); mean over bins; pad lag (+ n_fft // (2 hop) when centred) in front; trimmed to the F frames. numpy's mean adds in
    another order: within 256 e of the ordered sum."""
    F, D = 150, 40
    S = rm.rows(F, D, 3).astype(np.float64)
    ref = scipy.ndimage.maximum_filter1d(S, max_size, axis=1, mode="reflect")
    env = np.maximum(0.0, S[lag:] - ref[:-lag]).mean(axis=1)
    pad = lag + (n_fft // (2 * hop) if center else 0)
    want = np.concatenate([np.zeros(pad), env])[:F]
    got = rm.onset_strength64(S.astype(np.float32), lag=lag, max_size=max_size, n_fft=n_fft, hop=hop, center=center)
    assert got.shape == (F,) and np.all(np.abs(got - want) <= 256 * rm.E64 * np.abs(want))
    assert np.any(got > 0) or F <= pad


def test_short_segments_are_all_zeros_and_nonfinite_rows_flow():
    for F in (0, 1, 3, 4):
        assert np.array_equal(rm.onset_strength(rm.rows(F, 8, F), lag=2, n_fft=2048, hop=512), np.zeros(F, np.float32))  # p = 2
    S = rm.rows(6, 8, 9)
    S[2, 3], S[4, 1], S[5, 2] = np.nan, np.inf, -np.inf
    e = rm.onset_strength(S, lag=1, center=False)
    # a NaN shows as S (frame 2) and as R (frame 3); +Inf as S gives Inf (frame 4) and as R, against a finite S, clamps to 0 (frame 5);
    # -Inf as S clamps to 0 too
    assert e[0] == 0 and np.isfinite(e[1]) and np.isnan(e[2]) and np.isnan(e[3]) and np.isinf(e[4]) and np.isfinite(e[5])


# ---- onset frames ---------------------------------------------------------------------------------------------------------------
def _librosa_peak_pick(x, pre_max, post_max, pre_avg, post_avg, delta, wait):
    """librosa.util.peak_pick's loop (0.10.2, clipped windows), on the values onset_detect hands it."""
    peaks = np.zeros(len(x), bool)
    n = 0
    while n < len(x):
        maxn = np.max(x[max(0, n - pre_max):min(n + post_max, len(x))])
        peaks[n] = x[n] == maxn
        if not peaks[n]:
            n += 1
            continue
        avgn = np.mean(x[max(0, n - pre_avg):min(n + post_avg, len(x))])
        peaks[n] &= x[n] >= avgn + delta
        if not peaks[n]:
            n += 1
            continue
        n += wait + 1
    return np.flatnonzero(peaks)


CASES = rc.peak_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_peaks_in_librosas_words_and_decided(case, lib):
    """The model's list is librosa's loop on the normalised envelope; every comparison (b) is decided by more than its band; the
    library's window lengths are the model's."""
    _, x, rate, hop, times, delta, normalize = case
    w = rm.peak_windows(rate, hop, **times)
    spec = binding.OnsetPeaks(times["pre_max"], times["post_max"], times["pre_avg"], times["post_avg"], times["wait"], delta, hop, int(normalize))
    assert binding.onset_peak_windows(spec, rate) == w
    got, refused = rm.peak_pick(x, w, delta, normalize)
    assert not refused and len(got) <= -(-len(x) // (w[4] + 1))
    assert rm.band_b(x, w, delta, normalize) > 4.0
    u = rm._normalised(x, normalize)
    assert np.array_equal(got, _librosa_peak_pick(u, *w[:4], delta, w[4]))


def test_default_windows_and_the_constant_envelope_rule():
    assert rm.peak_windows(22050, 512) == (1, 1, 4, 5, 1)
    assert rm.peak_windows(44100, 512) == (2, 1, 8, 9, 2)
    w = rm.peak_windows(22050, 512)
    x = np.full(130, 0.5, np.float32)
    assert len(rm.peak_pick(x, w, 0.07)[0]) == 0
    assert np.array_equal(rm.peak_pick(x, w, 0.0)[0], np.arange(0, 130, w[4] + 1))
    x[17] = np.nan
    got, refused = rm.peak_pick(x, w, 0.0)
    assert refused and len(got) == 0


def test_click_train_onsets_are_the_clicks():
    x = rm.click_train()
    got, _ = rm.peak_pick(x, rm.peak_windows(22050, 512))
    assert np.array_equal(got, np.arange(5, 600, 20))


def test_peak_spec_refusals(lib):
    ok = dict(pre_max=0.03, post_max=0.0, pre_avg=0.1, post_avg=0.1, wait=0.03, delta=0.07, hop_length=512, options=1)
    for bad in (dict(pre_max=-1.0), dict(wait=np.nan), dict(post_avg=np.inf), dict(delta=np.inf), dict(hop_length=0), dict(options=2),
                dict(pre_avg=4097.0 * 512 / 22050)):
        with pytest.raises(binding.VsynError) as ei:
            binding.onset_peak_windows(binding.OnsetPeaks(**dict(ok, **bad)), 22050)
        assert ei.value.code == binding.VSYN_ERR_INVALID, bad
    assert binding.onset_peak_windows(binding.OnsetPeaks(**dict(ok, pre_avg=4096.0 * 512 / 22050 + 1e-9)), 22050)[2] == 4096


# ---- tempogram ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [2, 3, 16, 384, 689, 2048])
def test_window_and_padding_are_scipys_and_numpys(W):
    assert np.array_equal(rm.hann(W), scipy.signal.get_window("hann", W, fftbins=True).astype(np.float32))
    for F in (1, 2, W // 2 + 1, 300):
        e = rm.envelope(F, W + F, negative=True)
        assert np.array_equal(rm.pad_env(e, W), np.pad(e, W // 2, mode="linear_ramp", end_values=0))


@pytest.mark.parametrize("W,F,center", [(2, 5, True), (3, 7, True), (16, 40, False), (384, 30, True), (689, 700, False), (2048, 3, True)])
def test_tempogram_against_an_fft_autocorrelation(W, F, center):
    """librosa.autocorrelate: irfft(|rfft(y, 2 W - 1 padded)|^2)[:W], then util.normalize(norm=inf). The FFT route's own error is
    about log2(2 W) e sum y^2 per lag, far more than the direct sum's at a small |ac|: it is allowed on top of the model's bound."""
    e = rm.envelope(F, 31 * W + F)
    rows, bound = rm.tempogram(e, W, center, norm=True)
    Fp = rm.tg_rows(F, W, center)
    assert rows.shape == (Fp, W)
    ep = np.pad(e, W // 2, mode="linear_ramp", end_values=0).astype(np.float64) if center else e.astype(np.float64)
    win = scipy.signal.get_window("hann", W, fftbins=True).astype(np.float32).astype(np.float64)
    n = 1 << int(np.ceil(np.log2(2 * W)))
    for f in list(range(Fp))[:5] + list(range(Fp))[-3:]:
        y = win * ep[f:f + W]
        ac = np.fft.irfft(np.abs(np.fft.rfft(y, n)) ** 2, n)[:W]
        mx = np.abs(ac).max()
        want = ac / mx if mx > rm.FLT_MIN else ac
        fft_err = 8 * np.log2(n) * rm.E64 * np.sum(y * y) / max(mx, rm.FLT_MIN)
        assert np.all(np.abs(rows[f] - want) <= bound[f] + fft_err + rm.U32 * np.abs(want)), (W, f)
        assert mx <= rm.FLT_MIN or abs(rows[f, 0] - 1.0) < 1e-6


def test_tempogram_edges():
    assert rm.tempogram(rm.envelope(15, 1), 16, center=False)[0].shape == (0, 16)
    assert rm.tempogram(rm.envelope(16, 1), 16, center=False)[0].shape == (1, 16)
    rows, bound = rm.tempogram(np.zeros(9, np.float32), 8)
    assert not rows.any() and np.all(bound == rm.TINY)  # zero rows are not divided
    e = rm.envelope(40, 2)
    e[20] = np.nan
    rows, _ = rm.tempogram(e, 8)  # frame f reads e[f - 4 .. f + 3]
    assert np.array_equal(np.isnan(rows).all(axis=1), [17 <= f <= 24 for f in range(40)])
    assert not np.isnan(rows[~np.isnan(rows).all(axis=1)]).any()
    raw, _ = rm.tempogram(e, 8, norm=False)  # without the norm only the lags whose sum holds the NaN
    assert np.isnan(raw[17:25, 0]).all() and not np.isnan(raw[17:25]).all()


def test_tile_and_blocks_match_the_library(lib):
    for W in (2, 3, 16, 344, 384, 689, 1263, 1264, 2048):
        assert lib.vsyn_tempogram_tile(W) == rm.tg_tile(W)
        assert 8 * (2 * rm.tg_tile(W) + 1) * W <= max(79 * 1024, 8 * 9 * W)
    assert lib.vsyn_tempogram_tile(1) == 0 and lib.vsyn_tempogram_tile(2049) == 0
    assert rm.tg_blocks(600, 384) == (12, 50) and rm.tg_blocks(91136, 689) == (4 * 178, 128)
    spec = binding.TempogramSpec(0, 512, 3, 0, 8.0)
    assert lib.vsyn_tempogram_win_length(C.byref(spec), 22050) == 344 and lib.vsyn_tempogram_win_length(C.byref(spec), 44100) == 689
    assert lib.vsyn_tempogram_win_length(C.byref(spec), 192000) == 0  # 3000 frames
    assert lib.vsyn_tempogram_win_length(C.byref(binding.TempogramSpec(384, 512, 3, 0, 0.0)), 8000) == 384
    assert lib.vsyn_tempogram_win_length(C.byref(binding.TempogramSpec(0, 512, 3, 0, np.nan)), 22050) == 0
    r = np.random.default_rng(0).random((1000, 5)).astype(np.float32)
    assert np.allclose(rm.tg_mean(r), r.astype(np.float64).mean(axis=0), rtol=1e-13)
    assert np.isnan(rm.tg_mean(np.zeros((0, 4), np.float32))).all()


# ---- tempo ----------------------------------------------------------------------------------------------------------------------
def _librosa_tempo(tg_mean, sr, hop, start_bpm=120.0, std_bpm=1.0, max_tempo=320.0):
    """librosa.feature.tempo behind its mean: tempo_frequencies, the log-normal prior, the max_tempo mask, the arg-max."""
    bin_frequencies = np.zeros(len(tg_mean))
    bin_frequencies[0] = np.inf
    bin_frequencies[1:] = 60.0 * sr / (hop * np.arange(1.0, len(tg_mean)))
    logprior = -0.5 * ((np.log2(bin_frequencies) - np.log2(start_bpm)) / std_bpm) ** 2
    if max_tempo is not None:
        max_idx = int(np.argmax(bin_frequencies < max_tempo))
        logprior[:max_idx] = -np.inf
    best_period = np.argmax(np.log1p(1e6 * tg_mean) + logprior)
    return bin_frequencies[best_period], int(best_period)


TEMPO = rc.tempo_cases()


@pytest.mark.parametrize("case", TEMPO, ids=[c[0] for c in TEMPO])
def test_tempo_of_the_click_trains(case, lib):
    """The model, librosa's expressions and the library's host arithmetic agree, and the arg-max is decided beyond its band."""
    _, e, rate, hop, W, kw = case
    rows, _ = rm.tempogram(e, W)
    g = rm.tg_mean(rows)
    bpm, lag, margin, band = rm.tempo(g, rate, hop, **kw)
    assert margin > 1e3 * band > 0
    assert (bpm, lag) == _librosa_tempo(g, rate, hop, **kw)
    spec = binding.TempoSpec(kw.get("start_bpm", 120.0), kw.get("std_bpm", 1.0), kw.get("max_tempo", 320.0) or 0.0)
    assert binding.tempo_from_mean(spec, g, rate, hop) == (bpm, lag)


def test_click_train_tempo_is_its_period():
    e = rm.click_train()
    assert rm.tempo(rm.tg_mean(rm.tempogram(e, 384)[0]), 22050, 512)[:2] == (129.19921875, 20)
    assert rm.tempo(rm.tg_mean(rm.tempogram(rm.click_train(F=900, period=37, first=11), 689)[0]), 44100, 512)[1] == 37


def test_tempo_quirks_and_refusals(lib):
    g = np.zeros(16)
    g[3] = 1.0
    # no lag slower than max_tempo: nothing is masked (argmax of an all-false array is 0)
    assert rm.tempo(g, 22050, 512, max_tempo=1.0)[:2] == binding.tempo_from_mean(binding.TempoSpec(120.0, 1.0, 1.0), g, 22050, 512)
    assert rm.tempo(g, 22050, 512, max_tempo=1.0)[1] == 3
    # a tie goes to the first index, and lag 0 (-Inf) only wins when everything is -Inf: bpm +Inf
    z = np.zeros(4)
    assert binding.tempo_from_mean(binding.TempoSpec(120.0, 1.0, 0.0), z, 22050, 512)[1] == rm.tempo(z, 22050, 512, max_tempo=None)[1]
    ok = binding.TempoSpec(120.0, 1.0, 320.0)
    for bad_g in (np.array([0.0, np.nan, 1.0]), np.array([0.0, np.inf]), np.array([0.0, -1e-3, 1.0])):
        with pytest.raises(binding.VsynError):
            binding.tempo_from_mean(ok, bad_g, 22050, 512)
    for bad in (binding.TempoSpec(0.0, 1.0, 320.0), binding.TempoSpec(120.0, -1.0, 320.0), binding.TempoSpec(120.0, 1.0, -5.0),
                binding.TempoSpec(np.nan, 1.0, 320.0)):
        with pytest.raises(binding.VsynError):
            binding.tempo_from_mean(bad, g, 22050, 512)
    with pytest.raises(binding.VsynError):
        binding.tempo_from_mean(ok, np.zeros(1), 22050, 512)


def test_tempogram_inputs_decide_the_norm_threshold():
    """Every tempogram input of the GPU tests has its largest |ac| far from FLT_MIN, or exactly 0."""
    for W in (2, 3, 16, 384):
        for F in (1, W // 2 + 1, W):
            assert rm.tg_norm_margin(rm.envelope(F, 1000 + W + F), W) > 1e-20
            assert rm.tg_norm_margin(rm.envelope(F, 1000 + W + F, negative=True), W) > 1e-20
    assert rm.tg_norm_margin(np.zeros(9, np.float32), 8) == np.inf


# ---- rhythm.py ------------------------------------------------------------------------------------------------------------------
def test_rhythm_arguments_are_checked_before_the_library_loads(monkeypatch):
    from parseoggvorbis_amd import _corpus, rhythm

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_corpus, "load", no_load)
    blob = [b"x"]
    bad = [
        (rhythm.get_onset_strength_batch, dict(lag=0)), (rhythm.get_onset_strength_batch, dict(lag=65)),
        (rhythm.get_onset_strength_batch, dict(max_size=0)), (rhythm.get_onset_strength_batch, dict(max_size=2.0)),
        (rhythm.get_onset_strength_batch, dict(delta=1)), (rhythm.get_onset_strength_batch, dict(normalize="mean")),
        (rhythm.get_onset_strength_batch, dict(kind="lin_power")), (rhythm.get_onset_strength_batch, dict(kind="stft", n_fft=64)),
        (rhythm.get_onset_strength_batch, dict(kind="mel_power", n_mels=257)), (rhythm.get_onset_strength_batch, dict(no_such=1)),
        (rhythm.get_onset_strength_batch, dict(kind="mel_db", pcen=True)),
        (rhythm.get_onsets_batch, dict(pre_max=-0.1)), (rhythm.get_onsets_batch, dict(wait=np.inf)), (rhythm.get_onsets_batch, dict(delta=np.nan)),
        (rhythm.get_onsets_batch, dict(normalize=1)), (rhythm.get_onsets_batch, dict(envelope=())),
        (rhythm.get_tempogram_batch, dict(win_length=1)), (rhythm.get_tempogram_batch, dict(win_length=2049)),
        (rhythm.get_tempogram_batch, dict(win_length=None)), (rhythm.get_tempogram_batch, dict(norm=2)),
        (rhythm.get_tempogram_batch, dict(tg_center=None)),
        (rhythm.get_tempo_batch, dict(ac_size=0.0)), (rhythm.get_tempo_batch, dict(start_bpm=0.0)), (rhythm.get_tempo_batch, dict(std_bpm=-1.0)),
        (rhythm.get_tempo_batch, dict(max_tempo=np.inf)), (rhythm.get_tempo_batch, dict(tempogram_mean={})),
    ]
    for fn, kw in bad:
        with pytest.raises(rhythm.RhythmError):
            fn(blob, **kw)
    with pytest.raises(ValueError):
        rhythm.get_onset_strength_batch(blob, errors="ignore")
    with pytest.raises(AssertionError, match="loaded"):  # and a good call gets as far as the library
        rhythm.get_onset_strength_batch(blob, kind="mel_power", n_mels=256, hpss="percussive", lag=64, max_size=64)
    assert issubclass(rhythm.RhythmError, RuntimeError)


def test_rhythm_specs_mirror_the_header():
    from parseoggvorbis_amd import rhythm
    assert (C.sizeof(binding.OnsetSpec), C.sizeof(binding.OnsetPeaks), C.sizeof(binding.TempogramSpec), C.sizeof(binding.TempoSpec),
            C.sizeof(binding.RhythmSpec)) == (20, 56, 24, 24, 112)
    assert binding.RhythmSpec.peaks.offset == 32 and binding.RhythmSpec.tempogram.offset == 88
    t = rhythm.tempogram_spec(win_length=None, ac_size=8.0)
    assert (t.win_length, t.options, t.ac_size) == (0, 3, 8.0)
    assert rhythm.tempo_spec(max_tempo=None).max_tempo == 0.0
    p = rhythm.peaks_spec()
    assert binding.onset_peak_windows(p, 22050) == (1, 1, 4, 5, 1)
