"""The pyin stage on the CPU (include/vorbis_synth_hip.h, "pyin"): the float64 model (tests/pyin_model.py) against a restatement in
librosa's own words, the library's host-only transition table against the model's, the Python table of the Beta weights against
scipy, every check of step 10 on both sides of the C ABI, and that EVERY discrete decision of EVERY case of tests/pyin_cases.py
is decided, so that tests/test_gpu_pyin.py may ask for equal states on every frame."""
import ctypes
import math

import numpy as np
import pytest

from parseoggvorbis_amd import pitch
from tests import pitch_model as pm
from tests import pyin_cases as yc
from tests import pyin_model as ym
from tests import trim_model as tm

scipy_stats = pytest.importorskip("scipy.stats")


# ---- the model against a restatement in librosa's words ----

def _viterbi_as_librosa(prob, transition, p_init):
    """librosa.sequence.viterbi (prob (S, T)) with its _viterbi helper: log domain, np.argmax per target, backtracking."""
    eps = np.finfo(prob.dtype).tiny
    log_trans, log_prob, log_p_init = np.log(transition + eps), np.log(prob.T + eps), np.log(p_init + eps)
    n_steps, n_states = log_prob.shape
    value, ptr, state = np.zeros((n_steps, n_states)), np.zeros((n_steps, n_states), int), np.zeros(n_steps, int)
    value[0] = log_prob[0] + log_p_init
    for t in range(1, n_steps):
        trans_out = value[t - 1] + log_trans.T
        for j in range(n_states):
            ptr[t, j] = np.argmax(trans_out[j])
            value[t, j] = log_prob[t, j] + trans_out[j, ptr[t][j]]
    state[-1] = np.argmax(value[-1])
    for t in range(n_steps - 2, -1, -1):
        state[t] = ptr[t + 1, state[t + 1]]
    return state


def _restated(case):
    """librosa.pyin's body (>= 0.10) on the model's c: np.less.outer, cumsum, scipy.stats.boltzmann.pmf and beta.cdf, np.kron, the
    dense Viterbi; with the uniform p_init and the switch matrix of the section."""
    y = tm.downmix(case["x"])
    L, H, sr, fmin, fmax = case["L"], case["H"], case["sr"], case["fmin"], case["fmax"]
    p_min, p_max = pm.periods(sr, fmin, fmax, L)
    bps, B = ym.num_bins(fmin, fmax, case["resolution"])
    thresholds = np.linspace(0, 1, yc.N_THRESHOLDS + 1)
    beta_probs = np.diff(scipy_stats.beta.cdf(thresholds, 2, 18))
    frames = pm.frames_of(y, L, H, True)
    yin_frames = np.stack([pm.cmnd(z, p_min, p_max)[0] for z in frames], axis=1)  # (n, F)
    shifts = np.stack([[ym.shift_of(c, i)["shift"] for i in range(c.shape[0])] for c in yin_frames.T], axis=1)
    yin_probs = np.zeros_like(yin_frames)
    for i, yin_frame in enumerate(yin_frames.T):
        is_trough = ym.trough_mask(yin_frame)
        (trough_index,) = np.nonzero(is_trough)
        if len(trough_index) == 0:
            continue
        trough_heights = yin_frame[trough_index]
        trough_thresholds = np.less.outer(trough_heights, thresholds[1:])
        trough_positions = np.cumsum(trough_thresholds, axis=0) - 1
        n_troughs = np.count_nonzero(trough_thresholds, axis=0)
        with np.errstate(all="ignore"):
            trough_prior = scipy_stats.boltzmann.pmf(trough_positions, 2, n_troughs)
        trough_prior[~trough_thresholds] = 0
        probs = trough_prior.dot(beta_probs)
        global_min = np.argmin(trough_heights)
        n_below = np.count_nonzero(~trough_thresholds[global_min, :])
        probs[global_min] += 0.01 * np.sum(beta_probs[:n_below])
        yin_probs[trough_index, i] = probs
    yin_period, frame_index = np.nonzero(yin_probs)
    f0_candidates = sr / (p_min + yin_period + shifts[yin_period, frame_index])
    bin_index = np.clip(np.round(12 * bps * np.log2(f0_candidates / fmin)), 0, B).astype(int)
    observation_probs = np.zeros((2 * B, yin_frames.shape[1]))
    observation_probs[bin_index, frame_index] = yin_probs[yin_period, frame_index]
    voiced_prob = np.clip(np.sum(observation_probs[:B, :], axis=0, keepdims=True), 0, 1)
    observation_probs[B:, :] = (1 - voiced_prob) / B
    w = ym.width(sr, H, 35.92, bps)
    transition = np.kron(np.array([[0.99, 0.01], [0.01, 0.99]]), ym.loc_matrix(B, w))
    states = _viterbi_as_librosa(observation_probs, transition, np.full(2 * B, 1.0 / (2 * B)))
    return observation_probs[:B].T, voiced_prob[0], states


@pytest.mark.parametrize("k", [k for k, c in enumerate(yc.cases()) if c["T"] >= c["L"] and (c["group"] != "default" or c["T"] <= yc.T_MID)])
def test_the_model_against_a_restatement_in_librosas_words(k):
    """Observations within 1e-12 relative (a BLAS dot and a pairwise sum against the model's chains), the same candidates, the same
    states on every frame."""
    case = yc.cases()[k]
    table = np.diff(scipy_stats.beta.cdf(np.linspace(0, 1, yc.N_THRESHOLDS + 1), 2, 18))  # (the restatement's own table, bit for bit)
    m = ym.pyin(tm.downmix(case["x"]), case["sr"], case["fmin"], case["fmax"], table, case["L"], case["H"], resolution=case["resolution"])
    obs, vp, states = _restated(case)
    assert np.array_equal(obs > 0, m["obs"] > 0)
    assert np.allclose(obs, m["obs"], rtol=1e-12, atol=0) and np.allclose(vp, m["vp"], rtol=1e-12, atol=1e-15)
    assert np.array_equal(states, m["states"]), (case["group"], case["kind"], np.flatnonzero(states != m["states"])[:5])


def test_the_thresholds_and_the_triangle_are_numpys_and_scipys_bits():
    import scipy.signal
    for N in (1, 2, 3, 7, 49, 100, 1000, 1024):
        assert np.array_equal(ym.thresholds(N), np.linspace(0, 1, N + 1)[1:])
    assert not np.array_equal(np.arange(1, 50) / 49.0, np.linspace(0, 1, 50)[1:])  # (m / N is not)
    for w in (1, 3, 21, 101, 281):
        assert np.array_equal(ym.triangle(w), scipy.signal.get_window("triangle", w, fftbins=False))
    for B, w in ((12, 3), (25, 21), (71, 71), (60, 31), (59, 59)):
        assert np.array_equal(ym.loc_librosa(B, w), ym.loc_formula(B, w)) or np.allclose(ym.loc_librosa(B, w), ym.loc_formula(B, w), rtol=2e-16, atol=0)
        assert np.array_equal(ym.loc_librosa(B, w) > 0, ym.loc_formula(B, w) > 0)


def test_the_python_table_for_2_18_against_scipy():
    """The exact binomial sum is within 1.2e-15 of scipy.stats.beta.cdf at every threshold; the table is its differences."""
    for N in (1, 10, 100, 1024):
        x = np.linspace(0, 1, N + 1)
        cdf = np.array([0.0] + [pitch._beta_cdf_int(float(t), 2, 18) for t in x[1:-1]] + [1.0])
        assert np.abs(cdf - scipy_stats.beta.cdf(x, 2, 18)).max() <= 1.2e-15
        got = pitch.beta_probs(N, (2, 18))
        assert got.dtype == np.float64 and got.shape == (N,) and (got >= 0).all() and np.array_equal(got, np.diff(np.maximum.accumulate(np.clip(cdf, 0, 1))))
        assert np.abs(got - np.diff(scipy_stats.beta.cdf(x, 2, 18))).max() <= 2.4e-15
    frac = pitch.beta_probs(50, (2.5, 17.0))  # (not integers: scipy.special.betainc)
    assert np.abs(frac - np.diff(scipy_stats.beta.cdf(np.linspace(0, 1, 51), 2.5, 17.0))).max() <= 1e-14
    assert np.abs(pitch.beta_probs(100, (3, 4)) - np.diff(scipy_stats.beta.cdf(np.linspace(0, 1, 101), 3, 4))).max() <= 4e-15


def test_importing_the_package_imports_no_scipy():
    import subprocess
    import sys
    code = "import sys; import parseoggvorbis_amd, parseoggvorbis_amd.pitch; sys.exit(1 if any(m.split('.')[0] == 'scipy' for m in sys.modules) else 0)"
    assert subprocess.run([sys.executable, "-c", code], cwd=yc.__file__.rsplit("/tests/", 1)[0]).returncode == 0


# ---- every decision of every case ----

def test_every_decision_of_every_case_is_decided():
    """margin > band for every trough comparison, every h_k < t_m, the arg-min, every P_k > 0, every rint and clip of a bin, every
    back pointer on the optimal path and the final arg-max, in every case: the allowed share of undecided cases is zero. The decode
    alone (the model's obs through decode, the contract of vsyn_pyin_decode_device) is decided too."""
    for c, m in zip(yc.cases(), yc.models()):
        bad = [x for x in m["margins"] if not x[2] > x[3]]
        assert m["decided"] and not bad, (c["group"], c["kind"], c["T"], bad[:3])
        if len(m["states"]):
            assert m["dec"]["decided"], (c["group"], c["kind"], [x for x in m["dec"]["margins"] if not x[1] > x[2]][:3])


def test_the_cases_reach_their_branches():
    cs, ms = yc.cases(), yc.models()

    def of(group, kind):
        return [(c, m) for c, m in zip(cs, ms) if c["group"] == group and c["kind"] == kind and c["T"] >= c["L"]]
    c, m = of("default", "tone")[0]
    assert (m["B"], m["w"]) == (601, 101) and (m["vp"] == 1.0).sum() >= 10 and m["voiced"].sum() >= 20
    assert len(set(m["bins"][m["voiced"]])) >= 2  # both octaves are decoded
    for kind in ("zeros", "click"):  # no trough at all, all-equal unvoiced values
        c, m = of("default", kind)[0]
        assert all(len(f["lags"]) == 0 for f in m["frames"]) and not m["voiced"].any() and (m["vp"] == 0).all()
    c, m = of("default", "noise")[0]
    assert max(len(f["lags"]) for f in m["frames"]) > 100
    assert any((f["h"] >= 1.0).all() and (f["P"] > 0).sum() == 1 for f in m["frames"])  # only the no-trough term
    c, m = of("default", "periodic")[0]
    assert any((f["h"] == 0.0).any() for f in m["frames"])  # h = 0 < t_1 with band 0
    c, m = of("narrow", "tone")[0]
    assert m["B"] == 59 and m["w"] == 71 and len(m["states"]) == 235  # B < w: no out-of-band state
    assert [x["w"] for x in ms if x["B"] == 59 and x["w"] != 71][0] == 31
    c, m = of("small", "tone")[0]
    assert (m["B"], m["w"]) == (12, 3)
    step = np.abs(np.diff(m["bins"]))
    assert (step > 1).any()  # the decoded path itself leaves the band
    c, m = of("coarse", "noise")[0]
    shared = [np.bincount(f["bins"][(f["P"] > 0) & (f["bins"] < m["B"])], minlength=m["B"]).max() for f in m["frames"] if len(f["lags"])]
    assert m["bps"] == 2 and max(shared) >= 2  # two troughs share a bin: the last one wins
    c, m = [x for x in of("top", "tone") if x[1]["frames"][5]["bins"].max() == x[1]["B"]][0]
    assert any((f["bins"] == m["B"]).any() for f in m["frames"])  # a candidate lands on bin == B and is dropped
    c, m = [x for x in of("top", "tone") if not x[1]["frames"][5]["bins"].max() == x[1]["B"]][0]
    assert any(((f["x"] < 0) & (f["bins"] == 0)).any() for f in m["frames"])  # f0 < fmin, clipped to bin 0
    assert {c["C"] for c in cs} == {1, 2, 3}
    for grp in ("default", "narrow", "small"):
        assert len({c["sr"] for c in cs if c["group"] == grp}) == 2
        g = yc.GROUPS[grp]
        assert {g["H"] - 1, g["L"]} | ({0, 1, yc.T_MID} if grp == "default" else set()) <= {x["T"] for x in cs if x["group"] == grp}


# ---- the library's host-only table against the model ----

@pytest.fixture(scope="module")
def lib():
    from parseoggvorbis_amd import binding
    return binding.load()


def _transition(lib, spec, sr):
    w, B = ctypes.c_uint32(0), ctypes.c_uint32(0)
    err = ctypes.c_char_p()
    rc = lib.vsyn_pyin_transition(ctypes.byref(spec), sr, ctypes.byref(w), ctypes.byref(B), None, 0, ctypes.byref(err))
    if rc:
        return rc, w.value, B.value, None, err.value
    tab = np.full((B.value, w.value, 2), np.nan)
    rc = lib.vsyn_pyin_transition(ctypes.byref(spec), sr, None, None, tab.ctypes.data, tab.size, ctypes.byref(err))
    return rc, w.value, B.value, tab, err.value


# (sr, H, fmin, fmax, resolution): w in {1, 3, 101, 71, 31, 281}, B below, equal to and above w; then the sizes of
# tests/pyin_regime_cases.py: (B, w) = (1201, 201), (2048, 341), (59, 141), (36, 71), (37, 71)
TABLES = [(22050, 16, 1000.0, 1400.0, 0.5), (8000, 16, 400.0, 550.0, 0.5), (22050, 512, yc.C2, yc.C7, 0.1), (8000, 128, 200.0, 280.0, 0.1),
          (8000, 128, 200.0, 300.5, 0.1), (16000, 128, 200.0, 280.0, 0.1), (8000, 512, yc.C2, yc.C7, 0.1), (22050, 512, 30.0, 60.0, 0.5),
          (22050, 512, yc.C2, yc.C7, 0.05), (22050, 512, yc.C2, yc.C2 * 2.0 ** (2047.5 / 408.0), 0.03), (8000, 256, 200.0, 280.0, 0.1),
          (8000, 128, 200.0, 245.0, 0.1), (8000, 128, 200.0, 247.0, 0.1)]
# (sr, H, fmin, fmax, resolution, max_transition_rate, switch_prob): (601, 1) needs another rate; the other switch probabilities
TABLES_MORE = [(22050, 512, yc.C2, yc.C7, 0.1, 1.0, 0.01), (8000, 128, 200.0, 302.0, 0.1, 35.92, 0.3), (8000, 16, 400.0, 550.0, 0.5, 35.92, 0.49),
               (16000, 128, 200.0, 302.0, 0.1, 35.92, 0.3)]


def _check_table(lib, sr, H, fmin, fmax, res, mtr=35.92, sw=0.01):
    spec = pitch.pyin_spec(fmin, fmax, 2048 if H == 512 else 512 if H in (128, 256) else 64, H, resolution=res, max_transition_rate=mtr, switch_prob=sw)
    rc, w, B, tab, err = _transition(lib, spec, sr)
    assert rc == 0, err
    bps, Bm = ym.num_bins(fmin, fmax, res)
    wm = ym.width(sr, H, mtr, bps)
    assert (w, B) == (wm, Bm) and B == lib.vsyn_pyin_num_bins(ctypes.byref(spec))
    want = ym.band_table(ym.log_transition(B, w, sw), B, w)
    inside = want != ym.LT
    h = w // 2
    j = np.arange(B)[:, None] + np.arange(w)[None, :] - h
    assert np.array_equal(inside[:, :, 0], (j >= 0) & (j < B)) and np.array_equal(inside[:, :, 0], inside[:, :, 1])
    assert (tab[~inside] == ym.LT).all()
    assert (np.abs(tab[inside] - want[inside]) <= 2.0 ** -50 * np.abs(want[inside])).all()
    return B, w


@pytest.mark.parametrize("sr,H,fmin,fmax,res", TABLES)
def test_the_transition_table_against_the_model(lib, sr, H, fmin, fmax, res):
    """Relative 2^-50 inside the band, log(tiny) exactly outside it, w and B equal. (This test fails without the feature: the symbol
    does not exist.)"""
    _check_table(lib, sr, H, fmin, fmax, res)


@pytest.mark.parametrize("sr,H,fmin,fmax,res,mtr,sw", TABLES_MORE)
def test_the_transition_table_at_other_rates_and_switch_probabilities(lib, sr, H, fmin, fmax, res, mtr, sw):
    """The same comparison where max_transition_rate and switch_prob are not the defaults: w = 1 at B = 601, and the stay and switch
    entries at 0.3 and 0.49, which differ from each other by less than at 0.01."""
    B, w = _check_table(lib, sr, H, fmin, fmax, res, mtr, sw)
    assert (B, w) in ((601, 1), (72, 71), (12, 3), (72, 31))


def test_the_widths_and_sizes_of_the_tables_cover_the_section():
    got = set()
    for sr, H, fmin, fmax, res in TABLES:
        bps, B = ym.num_bins(fmin, fmax, res)
        w = ym.width(sr, H, 35.92, bps)
        got.add((w, "below" if B < w else "equal" if B == w else "above"))
    assert {w for w, _ in got} >= {1, 3, 101} and {r for _, r in got} == {"below", "equal", "above"}


def test_an_even_width_and_a_short_table_are_refused(lib):
    spec = pitch.pyin_spec(200.0, 280.0, 512, 128, resolution=0.3)  # bps = 4, msf = 7 at 8000 Hz: w = 29; msf = 3 at 16000 Hz: w = 13
    assert _transition(lib, spec, 8000)[:3] == (0, 29, ym.num_bins(200.0, 280.0, 0.3)[1])
    spec = pitch.pyin_spec(200.0, 280.0, 512, 128, resolution=0.5, max_transition_rate=40.0)  # bps = 2, msf = round(7.68) = 8: w = 17
    assert _transition(lib, spec, 8000)[1] == 17
    spec = pitch.pyin_spec(200.0, 280.0, 512, 128, resolution=0.34)  # bps = 3, msf = 7: w = 22
    rc, w, B, tab, err = _transition(lib, spec, 8000)
    assert rc == 1 and tab is None and b"odd" in err
    spec = pitch.pyin_spec(200.0, 280.0, 512, 128)
    tab = np.full(10, 7.0)
    err = ctypes.c_char_p()
    assert lib.vsyn_pyin_transition(ctypes.byref(spec), 8000, None, None, tab.ctypes.data, tab.size, ctypes.byref(err)) == 1 and (tab == 7.0).all()
    assert lib.vsyn_pyin_transition(ctypes.byref(spec), 0, None, None, None, 0, ctypes.byref(err)) == 1
    assert lib.vsyn_pyin_transition(ctypes.byref(spec), 500, None, None, None, 0, ctypes.byref(err)) == 1  # fmax above sr / 2


# ---- step 10 on both sides of the C ABI ----

GOOD = dict(fmin=65.0, fmax=2093.0, frame_length=2048, hop_length=512, n_thresholds=100, beta_parameters=(2, 18), boltzmann_parameter=2,
            resolution=0.1, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01, center=True)
BAD_ARGS = [dict(frame_length=3), dict(frame_length=8193), dict(frame_length=2048.0), dict(hop_length=0), dict(fmin=0.0), dict(fmin=-5.0),
            dict(fmin=500.0, fmax=400.0), dict(fmin=math.nan), dict(fmax=math.inf), dict(center=1), dict(n_thresholds=0), dict(n_thresholds=1025),
            dict(n_thresholds=10.0), dict(beta_parameters=(0, 18)), dict(beta_parameters=(2, -1)), dict(beta_parameters=2), dict(beta_parameters=(2, math.nan)),
            dict(boltzmann_parameter=0), dict(boltzmann_parameter=-1.0), dict(boltzmann_parameter=math.inf), dict(resolution=0.0), dict(resolution=1.0),
            dict(resolution=1), dict(resolution=math.nan), dict(max_transition_rate=0.0), dict(max_transition_rate=math.inf), dict(switch_prob=0.0),
            dict(switch_prob=1.0), dict(switch_prob=math.nan), dict(no_trough_prob=-0.1), dict(no_trough_prob=1.1), dict(no_trough_prob=math.nan),
            dict(fmin=20.0, fmax=8000.0, resolution=0.01)]  # (the last: 103 * 12 * 8.6 bins, above the states cap)


@pytest.mark.parametrize("kw", BAD_ARGS, ids=lambda kw: ",".join("%s=%r" % i for i in kw.items()))
def test_every_argument_is_checked_before_the_library_loads(kw, monkeypatch):
    def no_load():
        raise AssertionError("library loaded before the arguments were checked")
    monkeypatch.setattr(pitch, "_load", no_load)
    with pytest.raises(pitch.PyinError):
        pitch.pyin_spec(**dict(GOOD, **kw))
    with pytest.raises(pitch.PyinError):
        pitch.get_pyin_batch([b"OggS"], **dict(GOOD, **kw))
    with pytest.raises(pitch.PyinError):
        pitch.get_pyin_from_raw_bytes(b"OggS", **dict(GOOD, **kw))


def test_fill_na_sr_and_errors_are_checked_before_the_library_loads(monkeypatch):
    monkeypatch.setattr(pitch, "_load", lambda: (_ for _ in ()).throw(AssertionError("library loaded")))
    for kw in (dict(fill_na="nan"), dict(fill_na=True), dict(sr=0), dict(sr=22050.5)):
        with pytest.raises(pitch.PyinError):
            pitch.get_pyin_batch([b"OggS"], **dict(GOOD, **kw))
    with pytest.raises(ValueError):
        pitch.get_pyin_batch([b"OggS"], errors="ignore", **GOOD)


def test_a_non_integer_beta_without_scipy_raises(monkeypatch):
    import builtins
    real = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.split(".")[0] == "scipy":
            raise ImportError("no scipy here")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_scipy)
    with pytest.raises(pitch.PyinError, match="scipy"):
        pitch.beta_probs(10, (2.5, 18))
    assert pitch.beta_probs(10, (2, 18)).shape == (10,)  # (integers need none)


def _c_spec(**kw):
    from parseoggvorbis_amd.binding import PyinSpec
    a = dict(L=2048, H=512, options=1, N=100, fmin=65.0, fmax=2093.0, lam=2.0, res=0.1, mtr=35.92, sw=0.01, ntp=0.01, probs=pitch.beta_probs(100))
    a.update(kw)
    p = a["probs"]
    spec = PyinSpec(a["L"], a["H"], a["options"], a["N"], a["fmin"], a["fmax"], a["lam"], a["res"], a["mtr"], a["sw"], a["ntp"], None if p is None else p.ctypes.data)
    spec.probs = p
    return spec


def _probs(i, v):
    p = pitch.beta_probs(100).copy()
    p[i] = v
    return p


BAD_SPECS = [dict(L=3), dict(L=8193), dict(H=0), dict(options=2), dict(fmin=0.0), dict(fmin=-5.0), dict(fmin=500.0, fmax=400.0), dict(fmin=math.nan),
             dict(fmax=math.inf), dict(fmax=11026.0), dict(N=0), dict(N=1025), dict(probs=None), dict(probs=_probs(7, math.nan)), dict(probs=_probs(99, -1e-9)),
             dict(probs=_probs(0, math.inf)), dict(lam=0.0), dict(lam=-2.0), dict(lam=math.nan), dict(lam=math.inf), dict(res=0.0), dict(res=1.0),
             dict(res=math.nan), dict(mtr=0.0), dict(mtr=math.nan), dict(mtr=math.inf), dict(sw=0.0), dict(sw=1.0), dict(sw=math.nan), dict(ntp=-0.1),
             dict(ntp=1.1), dict(ntp=math.nan), dict(fmin=20.0, fmax=8000.0, res=0.01), dict(res=0.34, H=128, L=512, fmin=200.0, fmax=280.0)]
# (the last at 8000 Hz: w = 22, even)
BAD_SPECS.append(dict(res=0.03, fmax=yc.C2 * 2.0 ** (2048.5 / 408.0), fmin=yc.C2))  # B = 2049: one pair of states above the cap (B = 2048 passes)


@pytest.mark.parametrize("kw", BAD_SPECS, ids=lambda kw: ",".join("%s" % k for k in kw))
def test_every_check_of_step_10_through_the_c_entry(lib, kw):
    """VSYN_ERR_INVALID with a text, through the host-only entry, which runs the spec's and the rate's checks and touches no device."""
    err = ctypes.c_char_p()
    sr = 8000 if kw.get("res") == 0.34 else 22050
    assert lib.vsyn_pyin_transition(ctypes.byref(_c_spec()), 22050, None, None, None, 0, ctypes.byref(err)) == 0
    assert lib.vsyn_pyin_transition(ctypes.byref(_c_spec(**kw)), sr, None, None, None, 0, ctypes.byref(err)) == 1 and err.value
    if kw.get("res") != 0.34 and "fmax" not in kw or kw.get("fmax") != 11026.0 and kw.get("res") != 0.34:
        assert lib.vsyn_pyin_num_frames(ctypes.byref(_c_spec(**kw)), 100000) == 0 and lib.vsyn_pyin_num_bins(ctypes.byref(_c_spec(**kw))) == 0
    assert lib.vsyn_pyin_num_frames(ctypes.byref(_c_spec()), 22050) == 44 and lib.vsyn_pyin_num_frames(ctypes.byref(_c_spec()), 0) == 0


def test_the_spec_and_its_symbols_on_both_sides(lib):
    from parseoggvorbis_amd import binding
    assert ctypes.sizeof(binding.PyinSpec) == 80
    for name in ("vsyn_pyin_num_frames", "vsyn_pyin_num_bins", "vsyn_pyin_transition", "vsyn_pyin_device", "vsyn_pyin_decode_device", "vsyn_pcm_pyin_host"):
        assert name in binding.declared_symbols() and hasattr(lib, name)
    spec = pitch.pyin_spec(65.0, 2093.0)
    assert (spec.frame_length, spec.hop_length, spec.options, spec.n_thresholds) == (2048, 512, 1, 100)
    assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(spec.threshold_probs, ctypes.POINTER(ctypes.c_double)), (100,)), pitch.beta_probs(100))
