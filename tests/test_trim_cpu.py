"""The trim stage's float64 model (tests/trim_model.py) against an independent restatement in librosa's own words, its exact
properties, the margins of the GPU test's inputs, and the argument checks of get_pcm_batch / get_spectral_batch (raised before
the library is loaded). No GPU."""
import numpy as np
import pytest

from tests import trim_cases as tc
from tests import trim_model as tm


def librosa_trim(y, top_db, L, H):
    """librosa.effects.trim(y, top_db=top_db, ref=np.max, frame_length=L, hop_length=H) for a mono signal, in librosa's words:
    feature.rms(center=True, pad_mode="constant") over a strided view of the padded signal, amplitude_to_db(ref=np.max,
    amin=1e-5, top_db=None) > -top_db, frames_to_samples of the first and the last non-silent frame."""
    y = np.asarray(y, np.float64)
    T = y.shape[0]
    if T == 0:
        return 0, 0
    pad = np.pad(y, L // 2, mode="constant")
    if pad.shape[0] < L:
        return 0, 0
    frames = np.lib.stride_tricks.sliding_window_view(pad, L)[::H]
    rms = np.sqrt(np.mean(np.abs(frames) ** 2, axis=1))
    ref = rms.max()
    db = 20.0 * np.log10(np.maximum(1e-5, rms)) - 20.0 * np.log10(np.maximum(1e-5, ref))
    nz = np.flatnonzero(db > -top_db)
    if nz.size == 0:
        return 0, 0
    return int(nz[0]) * H, min(T, (int(nz[-1]) + 1) * H)


def _signal(rng, T, lead, tail, loud=0.2, quiet=1e-5):
    y = rng.standard_normal(T) * quiet
    y[lead:T - tail] = rng.standard_normal(max(T - tail - lead, 0)) * loud
    return y.astype(np.float32)


PARAMS = [(60.0, 2048, 512), (40.0, 400, 160), (20.0, 64, 16), (30.0, 7, 3), (50.0, 1, 1), (60.0, 16, 100), (60.0, 8192, 2048),
          (35.0, 401, 160)]


def test_model_equals_the_librosa_restatement():
    rng = np.random.default_rng(3)
    n = 0
    for top_db, L, H in PARAMS:
        for T in (1, 2, H - 1, H, H + 1, L, 3 * L + 5, 30011):
            if T < 1:
                continue
            for lead, tail in ((0, 0), (T // 3, T // 4), (T // 2, 0), (0, T // 2), (T - 1, 0)):
                y = _signal(rng, T, lead, tail)
                m = tm.trim(y, top_db, L, H)
                if m["margin"] <= 1e-6:  # (none does with this seed: asserted below)
                    continue
                n += 1
                assert (m["start"], m["end"]) == librosa_trim(y, top_db, L, H), (top_db, L, H, T, lead, tail)
                assert m["ms"].shape[0] == tm.num_frames(T, L, H)
    assert n == sum(5 for _, L, H in PARAMS for T in (1, 2, H - 1, H, H + 1, L, 3 * L + 5, 30011) if T >= 1)


def test_model_frame_sums_equal_fsum():
    rng = np.random.default_rng(4)
    for top_db, L, H in PARAMS:
        T = 2 * L + 3 * H + 1
        y = _signal(rng, T, T // 3, T // 4)
        ms = tm.frame_ms(y, L, H)
        for f in range(ms.shape[0]):
            want = tm.frame_ms_fsum(y, L, H, f)
            assert abs(ms[f] - want) <= 2.0 ** -52 * want, (L, H, f)


def test_bounds_are_multiples_of_the_hop_or_the_length():
    rng = np.random.default_rng(5)
    for top_db, L, H in PARAMS:
        for T in (1, H, H + 1, 5 * H + 7, 20011):
            y = _signal(rng, T, T // 3, T // 5)
            m = tm.trim(y, top_db, L, H)
            assert m["start"] % H == 0 and (m["end"] % H == 0 or m["end"] == T)
            assert 0 <= m["start"] < m["end"] <= T  # F >= 1: never trimmed to nothing


def test_silence_and_sub_amin_signals_are_returned_whole():
    rng = np.random.default_rng(6)
    for top_db, L, H in PARAMS:
        for T in (1, H + 1, 10007):
            for y in (np.zeros(T, np.float32), (rng.standard_normal(T) * 1e-6).astype(np.float32), np.full(T, 9e-6, np.float32)):
                m = tm.trim(y, top_db, L, H)
                assert (m["start"], m["end"]) == (0, T) and m["R"] == tm.AMIN_SQ
                assert (m["start"], m["end"]) == librosa_trim(y, top_db, L, H)


def test_a_power_of_two_scale_gives_the_same_bounds():
    rng = np.random.default_rng(7)
    for top_db, L, H in PARAMS:
        T = 20011
        y = _signal(rng, T, T // 3, T // 5, loud=0.2, quiet=2e-4)  # every frame stays above amin under 2^-3 as well
        m = tm.trim(y, top_db, L, H)
        for k in (-3, 3, 7):
            s = tm.trim(y * np.float32(2.0 ** k), top_db, L, H)
            assert s["R"] >= tm.AMIN_SQ and (s["start"], s["end"]) == (m["start"], m["end"])
            if s["ms"].min() > tm.AMIN_SQ and m["ms"].min() > tm.AMIN_SQ:
                assert np.array_equal(s["ms"], m["ms"] * 4.0 ** k)  # the sums scale exactly


def test_edge_lengths_odd_frames_and_hops_longer_than_the_frame():
    assert tm.num_frames(0, 2048, 512) == 0 and tm.num_frames(0, 7, 3) == 0
    m = tm.trim(np.zeros(0, np.float32), 60.0, 7, 3)
    assert (m["start"], m["end"], m["ms"].shape[0], m["R"]) == (0, 0, 0, tm.AMIN_SQ)
    rng = np.random.default_rng(8)
    for L, H in ((2048, 512), (7, 3), (401, 160), (16, 100), (1, 1)):
        for T in (0, 1, H - 1, H, H + 1):
            y = (rng.standard_normal(T) * 0.2).astype(np.float32)
            m = tm.trim(y, 60.0, L, H)
            F = tm.num_frames(T, L, H)
            assert m["ms"].shape[0] == F and (F >= 1) == (T >= 1)
            assert (m["start"], m["end"]) == librosa_trim(y, 60.0, L, H), (L, H, T)
            for f in range(F):
                assert abs(m["ms"][f] - tm.frame_ms_fsum(y, L, H, f)) <= 2.0 ** -52 * m["ms"][f]
    # H > L: the samples between the frames do not count
    y = np.zeros(1000, np.float32)
    y[150:190] = 0.5  # between frame 1 ([92, 108)) and frame 2 ([192, 208))
    m = tm.trim(y, 60.0, 16, 100)
    assert (m["start"], m["end"]) == (0, 1000) and not m["ms"].any()
    y[200] = 0.5
    m = tm.trim(y, 20.0, 16, 100)
    assert (m["start"], m["end"]) == (200, 300)
    # a sample that is not finite refuses the signal
    y[600] = np.inf
    m = tm.trim(y, 20.0, 16, 100)
    assert (m["start"], m["end"]) == (0, 0) and not np.isfinite(m["R"])


@pytest.mark.parametrize("L,H", tc.LH)
def test_the_gpu_cases_lie_outside_the_band(L, H):
    """Every input of tests/test_gpu_trim.py's per-value test has a model margin above (2L + 3) * 2^-53."""
    worst = float("inf")
    for Cn in tc.CHANNELS:
        for T, kind, x in tc.cases(Cn, L, H):
            m = tm.trim(tm.downmix(x) if T else np.zeros(0, np.float32), tc.TOP_DB, L, H)
            assert m["margin"] > tm.band(L), (Cn, L, H, T, kind, m["margin"])
            worst = min(worst, m["margin"])
            if kind in ("zeros", "sub_amin"):
                assert (m["start"], m["end"]) == (0, T)
            if kind == "from_0" and T:
                assert m["start"] == 0
            if kind == "last_hop" and T:
                assert m["end"] == T
    print("smallest margin (L %d, H %d): %.3g, band %.3g" % (L, H, worst, tm.band(L)))


def test_a_top_db_whose_threshold_rounds_to_the_maximum_keeps_the_loudest_frame():
    """k = 10^(-top_db / 10) rounds to 1 for a tiny top_db and R * k to R: the loudest frames are still non-silent (E >= R)."""
    rng = np.random.default_rng(9)
    y = _signal(rng, 5000, 1500, 1500)
    for top_db in (1e-300, 1e-17, 4e-16):
        m = tm.trim(y, top_db, 400, 160)
        f = int(np.argmax(m["ms"]))
        assert m["start"] <= f * 160 < m["end"] and m["end"] - m["start"] <= 160, (top_db, m["start"], m["end"])


# ---- the Python entry points' argument checks: raised before the library is loaded ----

@pytest.fixture()
def no_library(monkeypatch):
    from parseoggvorbis_amd import pcm, spectral

    def boom():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(pcm, "_load", boom)
    monkeypatch.setattr(spectral, "_load", boom)
    return pcm, spectral


BAD = [dict(trim_db="60"), dict(trim_db=True), dict(trim_db=[60.0]), dict(trim_db=0), dict(trim_db=-3.0), dict(trim_db=200.5),
       dict(trim_db=float("nan")), dict(trim_db=float("inf")), dict(trim_db=60.0, trim_frame_length=0),
       dict(trim_db=60.0, trim_frame_length=8193), dict(trim_db=60.0, trim_frame_length=2048.0), dict(trim_db=60.0, trim_hop_length=0),
       dict(trim_db=60.0, trim_hop_length=-1), dict(trim_db=60.0, trim_hop_length="512"), dict(trim_db=60.0, trim_index=())]


@pytest.mark.parametrize("kw", BAD, ids=[",".join("%s=%r" % i for i in kw.items()) for kw in BAD])
def test_bad_trim_arguments_are_refused_before_the_library_loads(no_library, kw):
    pcm, spectral = no_library
    with pytest.raises(pcm.PcmError):
        pcm.get_pcm_batch([b"x"], mono=True, **kw)
    with pytest.raises(spectral.SpectralError):
        spectral.get_spectral_batch([b"x"], **kw)


def test_trim_needs_mono(no_library):
    pcm, spectral = no_library
    from parseoggvorbis_amd.pcm import trim_spec
    assert trim_spec(None, 0, 0) is None  # the stage is off: its other arguments are not looked at
    assert trim_spec(60, 1, 2 ** 32 - 1).hop_length == 2 ** 32 - 1
    with pytest.raises(pcm.PcmError, match="mono=True"):
        pcm.get_pcm_batch([b"x"], trim_db=60.0)
    with pytest.raises(pcm.PcmError, match="mono=True"):
        pcm.get_pcm_batch([b"x"], mono=False, trim_db=60.0, trim_frame_length=400, trim_hop_length=160)
    for ok in (dict(trim_db=60.0), dict(trim_db=200), dict(trim_db=np.float32(0.5), trim_frame_length=8192, trim_hop_length=100000)):
        with pytest.raises(AssertionError, match="the library was loaded"):  # the checks pass: the next step is the load
            pcm.get_pcm_batch([b"x"], mono=True, **ok)
        with pytest.raises(AssertionError, match="the library was loaded"):
            spectral.get_spectral_batch([b"x"], **ok)
