"""The split stage's float64 model (tests/split_model.py) against an independent restatement in librosa's own words, the two forms
of the joined signal, the margins and the counts of the GPU test's inputs, and the argument checks of get_pcm_batch /
get_spectral_batch / get_intervals_batch (raised before the library is loaded). No GPU."""
import numpy as np
import pytest

from tests import split_cases as sc
from tests import split_model as sm
from tests import trim_model as tm
from tests.test_trim_cpu import PARAMS, _signal


def librosa_split(y, top_db, L, H):
    """librosa.effects.split(y, top_db=top_db, ref=np.max, frame_length=L, hop_length=H) for a mono signal, in librosa's words:
    _signal_to_frame_nonsilent (feature.rms(center=True, pad_mode="constant"), amplitude_to_db(ref=np.max, amin=1e-5, top_db=None)
    > -top_db), np.diff of the mask, the edge insertion, frames_to_samples, np.minimum(edges, T) and the reshape."""
    y = np.asarray(y, np.float64)
    T = y.shape[0]
    pad = np.pad(y, L // 2, mode="constant")
    if T == 0 or pad.shape[0] < L:
        return np.zeros((0, 2), np.int64)
    frames = np.lib.stride_tricks.sliding_window_view(pad, L)[::H]
    rms = np.sqrt(np.mean(np.abs(frames) ** 2, axis=1))
    db = 20.0 * np.log10(np.maximum(1e-5, rms)) - 20.0 * np.log10(np.maximum(1e-5, rms.max()))
    non_silent = db > -top_db
    edges = np.flatnonzero(np.diff(non_silent.astype(int)))
    edges = [edges + 1]
    if non_silent[0]:
        edges.insert(0, np.array([0]))
    if non_silent[-1]:
        edges.append(np.array([len(non_silent)]))
    edges = np.concatenate(edges) * H  # frames_to_samples
    edges = np.minimum(edges, T)
    return edges.reshape((-1, 2)).astype(np.int64)


def _gappy(rng, T, loud=0.2, quiet=1e-5):
    """Noise at `loud` in a few stretches of random length, noise at `quiet` between them."""
    y = rng.standard_normal(T) * quiet
    t = int(rng.integers(0, max(T // 7, 1) + 1))
    while t < T:
        n = int(rng.integers(1, max(T // 5, 2)))
        y[t:t + n] = rng.standard_normal(min(n, T - t)) * loud
        t += n + int(rng.integers(1, max(T // 5, 2)))
    return y.astype(np.float32)


def test_model_equals_the_librosa_restatement():
    rng = np.random.default_rng(13)
    n = several = 0
    for top_db, L, H in PARAMS:
        for T in (1, 2, H - 1, H, H + 1, L, 3 * L + 5, 30011):
            if T < 1:
                continue
            for y in (_gappy(rng, T), _gappy(rng, T), _signal(rng, T, T // 3, T // 4), _signal(rng, T, 0, T // 2), _signal(rng, T, T - 1, 0)):
                m = sm.split(y, top_db, L, H)
                assert m["margin"] > 1e-6, (top_db, L, H, T)  # (holds with this seed: a case inside would prove nothing)
                want = librosa_split(y, top_db, L, H)
                assert m["intervals"].shape == want.shape and np.array_equal(m["intervals"], want), (top_db, L, H, T)
                t = tm.trim(y, top_db, L, H)  # the first start and the last end are the trim's bounds
                assert (int(want[0, 0]), int(want[-1, 1])) == (t["start"], t["end"])
                n += 1
                several += len(want) > 2
    assert n == sum(5 for _, L, H in PARAMS for T in (1, 2, H - 1, H, H + 1, L, 3 * L + 5, 30011) if T >= 1) and several > 10


def test_degenerate_inputs():
    m = sm.split(np.zeros(0, np.float32), 60.0, 7, 3)
    assert m["intervals"].shape == (0, 2) and m["joined"].shape == (0,) and m["R"] == tm.AMIN_SQ and m["ms"].shape == (0,)
    rng = np.random.default_rng(14)
    for L, H in ((2048, 512), (7, 3), (16, 100), (1, 1)):
        for T in (1, H + 1, 10007):
            for y in (np.zeros(T, np.float32), (rng.standard_normal(T) * 1e-6).astype(np.float32)):
                m = sm.split(y, 60.0, L, H)
                assert m["intervals"].tolist() == [[0, T]] and np.array_equal(m["joined"], y)
                assert np.array_equal(m["intervals"], librosa_split(y, 60.0, L, H))
    y = np.zeros(1000, np.float32)
    y[200], y[600] = 0.5, np.inf
    m = sm.split(y, 20.0, 16, 100)
    assert m["intervals"].shape == (0, 2) and m["joined"].shape == (0,) and not np.isfinite(m["R"])
    # the last frame alone is non-silent and T is a multiple of H: an interval (T, T), as librosa lists it
    y = np.zeros(400, np.float32)
    y[396:] = 0.5
    m = sm.split(y, 20.0, 16, 100)
    assert m["intervals"].tolist() == [[400, 400]] and m["joined"].shape == (0,)
    assert np.array_equal(m["intervals"], librosa_split(y, 20.0, 16, 100))


@pytest.mark.parametrize("L,H", sc.LH)
def test_the_gpu_cases_lie_outside_the_band_and_reach_the_counts(L, H):
    """Every input of tests/test_gpu_split.py's per-value test: a model margin above (2L + 3) * 2^-53, both forms of the joined
    signal equal, n <= (F + 1) / 2; the nine signals shared with the trim stage are its segments, bit for bit. The counts the
    case set is there for: (16, 100) reaches n = (F + 1) / 2 = 501 of F = 1001 and an empty last interval (T, T); (1, 1) has tens
    of thousands of intervals at T = 100003 (the chunk carry of the device's scan); the smallest margin is about 4.6e-4."""
    from tests import trim_cases as tc
    worst, most, full, empty = float("inf"), 0, [], 0
    for Cn in sc.CHANNELS:
        both = sc.cases(Cn, L, H)
        for (T, kind, x), (T0, kind0, x0) in zip([c for c in both if c[1] in tc.SIGNALS], tc.cases(Cn, L, H)):
            assert (T, kind) == (T0, kind0) and np.array_equal(x.view(np.uint32), x0.view(np.uint32))
        assert len(both) == 10 * 12
        for T, kind, x in both:
            y = sm.downmix(x) if T else np.zeros(0, np.float32)
            m = sm.split(y, sc.TOP_DB, L, H)
            assert m["margin"] > sm.band(L), (Cn, L, H, T, kind, m["margin"])
            worst = min(worst, m["margin"])
            mask, _, _ = sm.loud_frames(m["ms"], sc.TOP_DB)
            F, n = mask.shape[0], len(m["intervals"])
            assert np.array_equal(sm.joined_by_hops(y, mask, H).view(np.uint32), m["joined"].view(np.uint32)), (Cn, L, H, T, kind)
            assert m["joined"].shape[0] == int((m["intervals"][:, 1] - m["intervals"][:, 0]).sum())
            assert n <= (F + 1) // 2 and (n >= 1) == (F >= 1)
            assert (m["intervals"][:-1, 1] % H == 0).all() and (m["intervals"][:, 0] % H == 0).all()  # only the last end is clipped
            if kind in ("zeros", "sub_amin") and T:
                assert m["intervals"].tolist() == [[0, T]]
            most = max(most, n)
            if n > 1 and n == (F + 1) // 2:
                full.append((T, kind, n, F))
            empty += n > 0 and int(m["intervals"][-1, 0]) == int(m["intervals"][-1, 1]) == T
    print("split cases (L %d, H %d): smallest margin %.3g, band %.3g, most intervals %d" % (L, H, worst, sm.band(L), most))
    assert worst > 4e-4
    if (L, H) == (16, 100):
        assert (100003, "alternate", 501, 1001) in full and empty >= 1
    if (L, H) == (1, 1):
        assert 45000 < most <= 50002
    if (L, H) == (400, 160):  # bursts: the gap shorter than a frame joins two of the four stretches
        assert len(sm.split(sm.downmix(sc.segment(1, "bursts", 1, 100003, L, H)), sc.TOP_DB, L, H)["intervals"]) == 3


# ---- the Python entry points' argument checks: raised before the library is loaded ----

@pytest.fixture()
def no_library(monkeypatch):
    from parseoggvorbis_amd import pcm, spectral

    def boom():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(pcm, "_load", boom)
    monkeypatch.setattr(spectral, "_load", boom)
    return pcm, spectral


BAD = [dict(split_db="60"), dict(split_db=True), dict(split_db=[60.0]), dict(split_db=0), dict(split_db=-3.0), dict(split_db=200.5),
       dict(split_db=float("nan")), dict(split_db=float("inf")), dict(split_db=60.0, split_frame_length=0),
       dict(split_db=60.0, split_frame_length=8193), dict(split_db=60.0, split_frame_length=2048.0), dict(split_db=60.0, split_hop_length=0),
       dict(split_db=60.0, split_hop_length=-1), dict(split_db=60.0, split_hop_length="512"), dict(split_db=60.0, split_index=()),
       dict(split_db=60.0, trim_db=60.0), dict(split_db=30.0, trim_db=60.0, trim_frame_length=400, trim_hop_length=160)]


@pytest.mark.parametrize("kw", BAD, ids=[",".join("%s=%r" % i for i in kw.items()) for kw in BAD])
def test_bad_split_arguments_are_refused_before_the_library_loads(no_library, kw):
    pcm, spectral = no_library
    with pytest.raises(pcm.PcmError, match="split_"):
        pcm.get_pcm_batch([b"x"], mono=True, **kw)
    with pytest.raises(spectral.SpectralError, match="split_"):
        spectral.get_spectral_batch([b"x"], **kw)


def test_split_needs_mono_and_the_interval_arguments(no_library):
    pcm, spectral = no_library
    assert pcm.split_spec(None, 0, 0) is None  # the stage is off: its other arguments are not looked at
    assert pcm.split_spec(60, 1, 2 ** 32 - 1).hop_length == 2 ** 32 - 1
    with pytest.raises(pcm.PcmError, match="mono=True"):
        pcm.get_pcm_batch([b"x"], split_db=60.0)
    with pytest.raises(pcm.PcmError, match="mono=True"):
        pcm.get_pcm_batch([b"x"], mono=False, split_db=60.0, split_frame_length=400, split_hop_length=160)
    for ok in (dict(split_db=60.0), dict(split_db=200, split_index=[]), dict(split_db=np.float32(0.5), split_frame_length=8192, split_hop_length=100000)):
        with pytest.raises(AssertionError, match="the library was loaded"):  # the checks pass: the next step is the load
            pcm.get_pcm_batch([b"x"], mono=True, **ok)
        with pytest.raises(AssertionError, match="the library was loaded"):
            spectral.get_spectral_batch([b"x"], **ok)
    for bad in (dict(top_db=None), dict(top_db="60"), dict(top_db=0), dict(top_db=201), dict(top_db=float("nan")), dict(frame_length=0),
                dict(frame_length=8193), dict(hop_length=0), dict(hop_length=1.5), dict(sr=0), dict(sr=16000.0)):
        with pytest.raises(pcm.PcmError):
            pcm.get_intervals_batch([b"x"], **bad)
    with pytest.raises(ValueError):
        pcm.get_intervals_batch([b"x"], errors="ignore")
    with pytest.raises(AssertionError, match="the library was loaded"):
        pcm.get_intervals_batch([b"x"], 40, 400, 160, sr=16000)
    with pytest.raises(AssertionError, match="the library was loaded"):
        pcm.get_intervals_from_raw_bytes(b"x")
