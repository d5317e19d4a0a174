"""The pitch stage without a GPU: the float64 model (tests/pitch_model.py) against a restatement in librosa's own words and
against math.fsum, the condition on the test inputs that lets tests/test_gpu_pitch.py demand every lag exactly, and the
argument checks of parseoggvorbis_amd.pitch, which run before the library is loaded."""
import numpy as np
import pytest

from parseoggvorbis_amd import pitch
from tests import pitch_cases as pc
from tests import pitch_model as pm
from tests import trim_model as tm


@pytest.mark.parametrize("L,H", pc.LH)
def test_model_agrees_with_the_fft_formulation(L, H):
    """(a) c of the model against librosa's route (rfft of the frame and of frame[W:0:-1], irfft, cumulative energies, cumulative
    mean) on the loud signals: 1e-10 absolute, above the error of a double FFT at L = 8192 and far below any decision gap. L = 8
    has too few lags for librosa's slicing to differ from the direct form; it is compared all the same."""
    worst = 0.0
    for c, m in zip(pc.cases(L, H), pc.models(L, H)):
        if c["kind"] not in pc.LOUD or c["T"] < L:
            continue
        z = pm.frames_of(tm.downmix(c["x"]), L, H)
        for f in sorted({0, len(z) // 2, len(z) - 1}):
            d = float(np.abs(pm.cmnd_fft(z[f], m["p_min"], m["p_max"]) - m["cs"][f]).max())
            print("fft", L, H, c["kind"], f, d)
            worst = max(worst, d)
            assert d <= 1e-10, (L, H, c["kind"], f, d)
    assert worst > 0.0


@pytest.mark.parametrize("L,H", pc.LH)
def test_model_difference_agrees_with_fsum(L, H):
    """(b) d of the model against the exactly rounded sum, on sampled frames and lags: equal to the last bit or one ulp away (the
    model rounds a longdouble sum once more)."""
    for c, m in zip(pc.cases(L, H), pc.models(L, H)):
        if c["T"] != pc.T_MID or c["kind"] in ("zeros",):
            continue
        z = pm.frames_of(tm.downmix(c["x"]), L, H)
        f = len(z) // 2
        for tau in sorted({1, m["p_min"], (m["p_min"] + m["p_max"]) // 2, m["p_max"]}):
            want = pm.difference_fsum(z[f], tau)
            got = float(m["d"][f][tau - 1])
            assert abs(got - want) <= 2.0 ** -52 * want, (L, H, c["kind"], tau, got, want)


@pytest.mark.parametrize("L,H", pc.LH)
def test_every_frame_decides_outside_the_band(L, H):
    """(c) every frame of every case has margin > band: a condition on the inputs, no frame left out. (d) |a| at i* is large
    enough that the bound on f0 stays under 1e-6 relative. Both branches of step 6 and both ends of the lag range occur."""
    branches, least = set(), np.inf
    for c, m in zip(pc.cases(L, H), pc.models(L, H)):
        F = pm.num_frames(c["T"], L, H)
        assert len(m["f0"]) == F == len(m["branch"])
        if F == 0:
            continue
        print("margin", L, H, c["kind"], c["C"], c["T"], c["sr"], float(m["margin"].min()), m["band"], float(m["tol"].max()))
        assert (m["margin"] > m["band"]).all(), (L, H, c["kind"], c["T"], float(m["margin"].min()), m["band"])
        assert (m["tol"] < 1e-6).all(), (L, H, c["kind"], c["T"], float(m["tol"].max()))
        branches |= set(m["branch"])
        least = min(least, float(m["margin"].min()))
        if c["kind"] == "zeros":
            assert (m["c"] == 0.0).all() and (m["f0"] == c["sr"] / m["p_min"]).all()  # step 8: (sr / p_min, 0) exactly
    assert branches == {"trough", "minimum"}
    assert least < 1.0


def test_periods_and_frame_counts():
    assert pm.periods(22050, 65.0, 2093.0, 2048) == (10, 340)
    assert pm.periods(44100, 10.0, 4000.0, 2048) == (11, 1023)  # the clamp L - W - 1
    assert pm.periods(8000, 2000.0, 4000.0, 8) == (2, 3)
    assert pm.periods(8000, 2000.0, 4000.0, 6) is None  # one lag: p_min = 2 = L - W - 1
    assert {len({pm.periods(c["sr"], c["fmin"], c["fmax"], L) for c in pc.cases(L, H)}) for L, H in pc.LH if L >= 64} == {3}
    for L, H in pc.LH:
        for T in pc.lengths(L, H):
            assert pm.num_frames(T, L, H) == (0 if T == 0 else 1 + T // H)  # L even: spec_num_frames with centre padding


BAD = [dict(fmin=0.0), dict(fmin=-1.0), dict(fmin=500.0, fmax=400.0), dict(fmin=400.0, fmax=400.0), dict(fmin=float("nan")),
       dict(fmax=float("inf")), dict(fmin="65"), dict(fmin=True), dict(frame_length=3), dict(frame_length=8193), dict(frame_length=2048.0),
       dict(frame_length=True), dict(hop_length=0), dict(hop_length=2 ** 32), dict(hop_length=1.5), dict(trough_threshold=0.0),
       dict(trough_threshold=1.5), dict(trough_threshold=float("nan")), dict(trough_threshold=None), dict(center=1), dict(sr=0),
       dict(sr=16000.0), dict(errors="ignore")]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join("%s=%r" % kv for kv in kw.items()))
def test_bad_arguments_are_refused_before_the_library_loads(kw, monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(pitch, "_load", no_load)
    args = dict(fmin=65.0, fmax=2093.0)
    args.update(kw)
    with pytest.raises((pitch.PitchError, ValueError)) as ei:
        pitch.get_f0_batch([b"x"], **args)
    assert "errors" in kw or isinstance(ei.value, pitch.PitchError)


def test_spec_defaults():
    s = pitch.pitch_spec(65.0, 2093.0)
    assert (s.frame_length, s.hop_length, s.options, s.fmin, s.fmax, s.trough_threshold) == (2048, 512, 1, 65.0, 2093.0, 0.1)
    s = pitch.pitch_spec(65, 2093, frame_length=1000, hop_length=None, center=False)
    assert (s.frame_length, s.hop_length, s.options) == (1000, 250, 0)
    assert issubclass(pitch.PitchError, RuntimeError)
