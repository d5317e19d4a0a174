"""The beat tracker's float64 model (tests/beat_model.py; include/vorbis_synth_hip.h, "rhythm", D) against an independent vectorised
restatement in numpy's and scipy's own words, the condition that every shared case (tests/beat_cases.py) decides every comparison by
more than its band, and the host-only pieces: vsyn_beat_period, the beat spec's refusals and its layout. No GPU."""
import ctypes as C

import numpy as np
import pytest
import scipy.signal

import __graft_entry__ as entry
from parseoggvorbis_amd import binding
from tests import beat_cases as bc
from tests import beat_model as bm
from tests import rhythm_model as rm


@pytest.fixture(scope="module")
def lib():
    entry.build_hip()
    return binding.load()


def restated(u, P, tightness, trim):
    """D.2 to D.5 on the normalised envelope, in the words of librosa's vectorised tracker: scipy's convolution, a candidate array a
    frame with numpy.argmax on the reversed window (the first of equal scores is then the largest loc, the smallest d),
    numpy.ma.median over the local maxima, numpy.convolve with numpy.hanning(5)."""
    F = len(u)
    w = np.exp(-0.5 * (np.arange(-P, P + 1) * 32.0 / P) ** 2)
    ls = scipy.signal.convolve(u, w, "same", method="direct")
    lo = max(int(np.rint(P / 2.0)), 1)
    window = np.arange(-2 * P, -lo + 1)  # loc - i, ascending
    txwt = -tightness * np.log(-window / float(P)) ** 2
    reach = ls >= 0.01 * ls.max()
    i0 = int(np.argmax(reach)) if reach.any() else F
    cum, back = np.zeros(F), np.full(F, -1, np.int32)
    for i in range(F):
        loc = i + window
        ok = loc >= 0
        if not ok.any():
            cum[i] = ls[i]
            continue
        cand = np.where(ok, cum[np.maximum(loc, 0)] + txwt, -np.inf)[::-1]
        k = int(np.argmax(cand))
        cum[i] = ls[i] + cand[k]
        if i >= i0:
            back[i] = loc[::-1][k]
    pad = np.pad(cum, 1, mode="edge")
    ismax = (cum > pad[:-2]) & (cum >= pad[2:])
    if not ismax.any():
        return ls, cum, back, np.zeros(0, np.int64)
    med = float(np.ma.median(np.ma.masked_array(cum, ~ismax)))
    good = np.flatnonzero(ismax & (cum >= 0.5 * med))
    tail = int(good[-1]) if len(good) else F - 1
    beats = [tail]
    while back[beats[-1]] >= 0:
        beats.append(int(back[beats[-1]]))
    beats = np.array(beats[::-1], np.int64)
    # (numpy's "same" is as long as the LONGER argument: with fewer than five beats scipy's, which librosa calls, keeps the beats' length)
    v = ls[beats]
    sm = np.convolve(v, np.hanning(5), "same") if len(v) >= 5 else scipy.signal.convolve(v, np.hanning(5), "same", method="direct")
    t = 0.5 * np.sqrt(np.mean(sm ** 2)) if trim else 0.0
    over = np.flatnonzero(ls > t)
    if not len(over):
        return ls, cum, back, np.zeros(0, np.int64)
    return ls, cum, back, beats[(beats >= over[0]) & (beats <= over[-1])]


@pytest.mark.parametrize("name", bc.names())
def test_case_is_decided_and_the_model_is_the_restatement(name):
    """Every comparison of the case is decided by more than its band (a condition: a case that does not decide is replaced in
    tests/beat_cases.py, never skipped), and the model's ls and cum lie within LSB and CB of the restatement's on the same u, its
    integers equal. scipy's direct convolution adds in another order: that is what LSB allows either chain."""
    _, x, P, tight, trim = bc.case(name)
    r = bc.model(name)
    assert r["refused"] == 0
    assert r["worst"] > 1.0, r["worst_at"]
    if not r["scored"]:
        assert len(r["beats"]) == 0 and (len(x) < 2 or not x.any())
        return
    F = len(x)
    sd = float(np.std(x.astype(np.float64), ddof=1))
    assert abs(sd - r["sd"]) <= (F + 8) * bm.E64 * sd  # numpy's pairwise order against the documented one
    ls, cum, back, beats = restated(r["u"], P, tight, trim)
    tiny = 2.0 ** -1022
    assert np.all(np.abs(ls - r["ls"]) <= r["LSB"] + tiny), float((np.abs(ls - r["ls"]) / (r["LSB"] + tiny)).max())
    assert np.all(np.abs(cum - r["cum"]) <= r["CB"] + tiny), float((np.abs(cum - r["cum"]) / (r["CB"] + tiny)).max())
    assert np.array_equal(back, r["back"])
    assert np.array_equal(beats, r["beats"])


def test_the_cases_cover_the_paths_they_are_there_for():
    assert [bm.half(P) for P in (1, 2, 3, 5, 7)] == [(0, 1), (1, 1), (2, 2), (2, 2), (4, 4)]  # half to even, and lo = max(h, 1)
    res = {n: bc.model(n) for n in bc.names()}
    odd = [n for n, r in res.items() if r["maxima"] % 2 == 1 and r["maxima"] > 1]
    even = [n for n, r in res.items() if r["maxima"] % 2 == 0 and r["maxima"] > 0]
    assert odd and even, (len(odd), len(even))
    assert res["constant"]["sd"] == 0.0 and res["constant_one"]["sd"] == 0.0 and res["constant_below_lo"]["sd"] == 0.0
    assert len(res["constant"]["beats"]) > 100 and np.all(res["constant_below_lo"]["back"] == -1) and np.all(res["below_lo"]["back"] == -1)
    for n in ("zeros", "one_frame", "no_frames"):
        assert not res[n]["scored"] and len(res[n]["beats"]) == 0
    # the plateau: equal neighbours in cum, the frame in front of them a local maximum by >=, the ones inside none by >
    p = res["plateau"]
    assert p["cum"][99] == p["cum"][100] == p["cum"][109] and p["cum"][98] < p["cum"][99] and p["cum"][109] < p["cum"][110]
    assert res["late_start"]["i0"] > 100 and np.all(res["late_start"]["back"][:res["late_start"]["i0"]] == -1)
    assert res["late_start"]["back"][res["late_start"]["i0"] + 40] >= 0
    # 30 beats: on the clicks up to the last one, which the walk reaches from the last frame (a local maximum by the edge rule)
    assert len(res["clicks20"]["beats"]) == 30 and np.array_equal(res["clicks20"]["beats"][:29], np.arange(5, 585, 20))
    assert len(res["many_steps"]["beats"]) > 900
    x = rm.envelope(70, 8)
    x[64] = np.nan
    assert bm.beat_track(x, 7)["refused"] == 1
    x[64] = np.inf
    assert bm.beat_track(x, 7)["refused"] == 1


def test_smallest_margins_and_the_size_of_the_bands():
    """The smallest relative arg-max margins of two everyday inputs (a click train, a random envelope) are of order 1e-5; the bounds
    on cum, which make the bands, stay below 1e-11 of the scores even after 20000 frames."""
    assert 2.0e-5 < bc.model("clicks20")["smallest_rel"] < 2.4e-5
    assert 3.5e-5 < bc.model("random_P11")["smallest_rel"] < 4.5e-5
    for n in ("clicks20", "clicks37", "random_P11", "many_steps"):
        r = bc.model(n)
        assert float((r["CB"] / np.maximum(np.abs(r["cum"]), 1e-300)).max()) < 1e-11


@pytest.mark.parametrize("P", [1, 2, 3, 5, 7, 64, 2048])
def test_tables(P):
    w = bm.window(P)
    assert len(w) == 2 * P + 1 and w[P] == 1.0 and np.array_equal(w, w[::-1])
    tx, txe = bm.transition(P, 100.0)
    assert tx[P] == 0.0 and txe[P] == 0.0 and np.all(tx <= 0.0) and tx[2 * P] == pytest.approx(-100.0 * np.log(2.0) ** 2)


# ---- the library's host arithmetic ----------------------------------------------------------------------------------------------------
def test_beat_period_is_the_models(lib):
    from parseoggvorbis_amd import rhythm
    for hop in (512, 160, 1):
        spec = rhythm.beat_spec(hop_length=hop)
        for rate in (8000, 22050, 44100, 48000):
            for bpm in (30.0, 60.0, 117.45383523, 120.0, 129.19921875, 143.5546875, 300.0, 1e-3, 1e7):
                assert binding.beat_period(spec, bpm, rate) == bm.period(bpm, rate, hop), (hop, rate, bpm)
    spec = rhythm.beat_spec(hop_length=1)
    assert binding.beat_period(spec, 60.0 * 2 / 5, 1) == 2 and binding.beat_period(spec, 60.0 * 2 / 7, 1) == 4  # 2.5 and 3.5: half to even
    assert binding.beat_period(spec, 60.0 / 2048, 1) == 2048 and binding.beat_period(spec, 60.0 / 2049, 1) == 0
    assert binding.beat_period(spec, 60.0, 1) == 1 and binding.beat_period(spec, 60.0 / 0.4, 1) == 0
    for bpm in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(binding.VsynError) as ei:
            binding.beat_period(spec, bpm, 22050)
        assert ei.value.code == binding.VSYN_ERR_INVALID
    with pytest.raises(binding.VsynError):
        binding.beat_period(spec, 120.0, 0)
    for field, v in (("tightness", 0.0), ("tightness", np.nan), ("start_bpm", -1.0), ("start_bpm", np.inf), ("bpm", -1.0), ("bpm", np.nan),
                     ("hop_length", 0), ("options", 2)):
        bad = rhythm.beat_spec()
        setattr(bad, field, v)
        with pytest.raises(binding.VsynError) as ei:
            binding.beat_period(bad, 120.0, 22050)
        assert ei.value.code == binding.VSYN_ERR_INVALID, field


def test_beat_spec_mirrors_the_header():
    from parseoggvorbis_amd import rhythm
    assert C.sizeof(binding.BeatSpec) == 32 and binding.BeatSpec.hop_length.offset == 24 and binding.BeatSpec.options.offset == 28
    s = rhythm.beat_spec()
    assert (s.tightness, s.start_bpm, s.bpm, s.hop_length, s.options) == (100.0, 120.0, 0.0, 512, binding.VSYN_BEAT_TRIM)
    s = rhythm.beat_spec(400.0, 90.0, 128.5, False, 160)
    assert (s.tightness, s.start_bpm, s.bpm, s.hop_length, s.options) == (400.0, 90.0, 128.5, 160, 0)
    for kw in (dict(tightness=0.0), dict(tightness=np.inf), dict(tightness="tight"), dict(start_bpm=0.0), dict(start_bpm=np.nan), dict(bpm=0.0),
               dict(bpm=-3.0), dict(bpm=np.inf), dict(trim=1), dict(hop_length=0), dict(hop_length=1.5)):
        with pytest.raises(rhythm.RhythmError):
            rhythm.beat_spec(**kw)
    assert {"vsyn_beat_period", "vsyn_beat_track_device", "vsyn_pcm_chain_beats_host"} <= set(binding.declared_symbols())


def test_beat_arguments_are_checked_before_the_library_loads(monkeypatch):
    from parseoggvorbis_amd import _corpus, rhythm

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_corpus, "load", no_load)
    blob = [b"x"]
    for kw in (dict(tightness=0.0), dict(tightness=np.nan), dict(start_bpm=-1.0), dict(bpm=0.0), dict(bpm=np.inf), dict(bpm=[120.0, 90.0]),
               dict(bpm=[-1.0]), dict(bpm="fast"), dict(trim=None), dict(lag=0), dict(max_size=65), dict(envelope=()), dict(delta=1),
               dict(normalize="mean"), dict(kind="lin_power"), dict(no_such=1), dict(bpm=[120.0], bpm_list=1)):
        with pytest.raises(rhythm.RhythmError):
            rhythm.get_beats_batch(blob, **kw)
    with pytest.raises(rhythm.RhythmError):
        rhythm.get_beats_from_raw_bytes(b"x", tightness=-1.0)
    with pytest.raises(ValueError):
        rhythm.get_beats_batch(blob, errors="ignore")
    for kw in (dict(), dict(bpm=120.0), dict(bpm=[90.0]), dict(kind="mel_power", n_mels=256, hpss="percussive", trim=False, tightness=400.0)):
        with pytest.raises(AssertionError, match="loaded"):  # a good call gets as far as the library
            rhythm.get_beats_batch(blob, **kw)
