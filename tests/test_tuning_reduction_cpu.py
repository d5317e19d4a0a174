"""The cases of tests/tuning_reduction_cases.py certified without a GPU, from the model alone (tests/tuning_model.py), so that
tests/test_gpu_tuning_reduction.py can demand equality with nothing left out:

  every crafted tone inside the band is a decided peak and its two neighbours are decided non-peaks under the decision bands of the
  linear spectra's bound (allowed share of undecided ones: zero), and the model's peaks are exactly the crafted tones;
  every case has the property it is named for: records per frame and n, the byte in which the two middle keys split (for the two
  high bytes at every magnitude inside the model's +- dmag), the selected count, equal counts in the tied bins, the winner in bin 0
  and in bin nbin - 1, every selected residual of a crafted segment at least 1e-5 from every edge, one admitted tuning, a frame at
  exactly cap;
  the host reduction (vsyn_pitch_tuning: tune_host) agrees with the model on every case's rows;
  vsyn_piptrack_tile is 1 at the two framings of group D."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as entry
from parseoggvorbis_amd import binding
from tests import tuning_model as tm
from tests import tuning_reduction_cases as rc


@pytest.fixture(scope="module")
def lib():
    entry.build_hip()
    return binding.load()


def check_claims(L, s, pitch, mag, reached, what):
    """What a segment claims, read from rows (the model's here, the device's in the GPU module). reached collects the classes."""
    p, c = rc.params(L), s["claim"]
    want = tm.pitch_tuning(pitch, mag, p["resolution"], p["bins_per_octave"])
    assert want["admitted"] == [want["tuning"]], (what, want)
    k = rc.klass(pitch, mag)
    reached.add(("klass", k))
    if "n" in c:
        assert want["n"] == c["n"], (what, want)
    if "F" in c:
        assert pitch.shape[0] == c["F"], (what, pitch.shape)
    if "klass" in c:
        assert k == c["klass"], (what, k)
    if "one_of" in c and k == c["one_of"]:
        reached.add(("one_of", k))
    if "selected" in c:
        assert want["selected"] == c["selected"], (what, want)
    counts, margin = rc.histogram(pitch, mag, p["resolution"], p["bins_per_octave"])
    win = rc.winners(counts)
    if want["n"]:
        assert (margin >= 1e-5 or s["frames"] is None) and counts.sum() == want["selected"] and want["tuning"] == tm.edges(p["resolution"])[win[0]], (what, margin, win)
    if "tied" in c:
        assert len(win) == c["tied"], (what, win, counts[win])
        reached.add(("tied", c["tied"]))
        if c["tied"] > 1 and counts.size > 256:
            reached.add(("far", "same thread" if (win[-1] - win[0]) % 256 == 0 else "first thread lower" if win[0] % 256 < win[1] % 256 else "first thread higher"))
    if c.get("first_bin"):
        assert win == [0], (what, win)
        reached.add(("bin", "first"))
    if c.get("last_bin"):
        assert win == [counts.size - 1], (what, win)
        reached.add(("bin", "last"))
    if c.get("at_cap"):
        full = int(rc.per_frame(pitch).max())
        assert full == rc.cap(L, s["sr"]), (what, full)
        reached.add(("cap", full))
    return want


ALL = [(g, L) for g, Ls in rc.launches().items() for L in Ls]


@pytest.mark.parametrize("group,L", ALL, ids=[L["name"] for _, L in ALL])
def test_every_case_is_decided_and_has_its_property(lib, group, L):
    p = rc.params(L)
    n_fft = L["n_fft"]
    reached = set()
    for s in L["segs"]:
        what = (L["name"], s["name"])
        S, dS, pitch, mag = rc.model_rows(L, s)
        if s["frames"] is not None:
            k_lo, k_hi = tm.bins(s["sr"], n_fft, p["fmin"], p["fmax"])
            want_peak = np.zeros(pitch.shape, bool)
            for f, tones in enumerate(s["frames"][:pitch.shape[0]]):
                for k, _ in tones:
                    assert 2 <= k <= n_fft // 2 - 2, what
                    want_peak[f, k] = k_lo <= k < k_hi
            assert np.array_equal(pitch > 0, want_peak), (what, np.argwhere((pitch > 0) != want_peak)[:4])
            D = tm.decisions(S, dS, s["sr"], n_fft, p["fmin"], p["fmax"], p["threshold"])
            near = want_peak | np.roll(want_peak, 1, axis=1) | np.roll(want_peak, -1, axis=1)
            undecided = near & ~D["peak"] & ~D["nonpeak"]
            assert not undecided.any(), (what, np.argwhere(undecided)[:4])
            assert D["peak"][want_peak].all() and not D["peak"][~want_peak].any(), what
            if s["claim"].get("klass") in (2, 3):  # the class holds wherever the device's magnitudes lie inside the model's band
                lo, hi = (D["mag"] - D["dmag"])[want_peak], (D["mag"] + D["dmag"])[want_peak]
                cut = np.median(D["mag"][want_peak])
                low, high = D["mag"][want_peak] < cut, D["mag"][want_peak] > cut
                assert low.sum() == high.sum() == want_peak.sum() // 2
                ends = {rc.split_byte(np.float32(a), np.float32(b)) for a in (lo[low].min(), hi[low].max()) for b in (lo[high].min(), hi[high].max())}
                assert ends == {s["claim"]["klass"]} and hi[low].max() < lo[high].min(), (what, ends)
        else:
            assert (pitch > 0).sum() > 0, what
        want = check_claims(L, s, pitch, mag, reached, what)
        for rows in ((pitch, mag), (pitch[::-1].copy(), mag[::-1].copy())):
            got = binding.pitch_tuning(rows[0], rows[1], p["resolution"], p["bins_per_octave"])
            assert got == (want["tuning"], want["n"], want["selected"]), (what, got, want)
    if group == "select" and L["power"] == 1:
        assert {("klass", 3), ("klass", 2), ("klass", "equal"), ("klass", "odd"), ("one_of", 1), ("one_of", 0)} <= reached, reached
    if L["name"] == "hist_4096_bins":
        assert {("far", "first thread lower"), ("far", "first thread higher"), ("tied", 3), ("bin", "first"), ("bin", "last")} <= reached, reached
    if L["name"] == "hist_same_thread":
        assert ("far", "same thread") in reached, reached
    if L["name"] in ("hist_0.01", "hist_0.3"):
        assert {("tied", 2), ("tied", 3), ("tied", 1), ("bin", "first"), ("bin", "last")} <= reached, reached
    if group == "cap":
        assert reached & {("cap", {"cap_512_default": 45, "cap_512_wide": 127, "cap_512_wide_p2": 127, "cap_64": 14}[L["name"]])}, reached


def test_the_searched_rates_and_the_sizes_the_cases_are_named_for():
    """The search of the issue redone: k = 5 at n_fft 64 has rates with residuals within 1e-4 of -0.5 and of +0.5; the record counts
    of group A straddle TUNE_WAVES; a dense frame of the wide band takes two lane strides."""
    lo, hi = rc.find_rate((5,), 0.01, near=-0.5), rc.find_rate((5,), 0.01, near=0.5)
    r = tm.residuals(np.array([5 * lo / 64.0, 5 * hi / 64.0], np.float32))
    assert -0.5 <= r[0] < -0.5 + 1e-4 and 0.5 - 1e-4 < r[1] < 0.5, (lo, hi, r)
    with open(entry.CSRC + "/vsyn_tuning.h") as f:
        text = f.read()
    assert "#define TUNE_THREADS 256\n" in text and "#define TUNE_WAVES (TUNE_THREADS / 64)\n" in text and rc.TUNE_WAVES == 4
    ns = {s["claim"]["n"] for s in rc.select_segments() if "n" in s["claim"]}
    assert {1, 2, 3, rc.TUNE_WAVES - 1, rc.TUNE_WAVES, rc.TUNE_WAVES + 1, 65} <= ns
    assert rc.cap(rc.launches()["cap"][1], rc.SR) == 127 > 64 and (512 // 2 + 1) % 64 == 1


def test_the_direct_kernel_takes_one_frame_a_workgroup_in_group_d(lib):
    """Beside test_tuning_cpu.py's test_the_models_tiles_are_the_librarys: the two framings of group D give tile 1 (8 n + 7 hop + 8
    floats do not fit the LDS), while the linear spectra's direct kernel still takes 8 frames at the first."""
    from parseoggvorbis_amd import spectral, tuning
    for n, hop, center in rc.TILE1:
        assert lib.vsyn_piptrack_tile(C.byref(tuning.framing_spec(n, hop, n, center))) == 1
        assert 8 * n + 7 * hop + 8 > 40960 >= 4 * n + n // 2 + 1
    assert lib.vsyn_spectral_lin_tile(C.byref(spectral.spectral_spec("lin_power", n_fft=4410, hop_length=1102, power=1))) == 8
