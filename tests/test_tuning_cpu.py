"""The tuning estimation without a GPU (include/vorbis_synth_hip.h, "tuning estimation"): the host-only reduction vsyn_pitch_tuning
against the model (tests/tuning_model.py) and against numpy.median / numpy.histogram, vsyn_piptrack_bins against the model, the
model's vectorised piptrack against a plain loop, every refusal of step 9 on both sides (in Python before the library loads, and
through the C functions), and what the GPU tests rely on: the chord's decision bands leave at most 1 % of the model's peaks undecided
at every framing of the GPU grid, and no selected residual of the chord sits on a histogram edge."""
import ctypes as C
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
from parseoggvorbis_amd import binding
from tests import spectral_lin_model as lm
from tests import tuning_model as tm


@pytest.fixture(scope="module")
def lib():
    entry.build_hip()
    return binding.load()


def numpy_tuning(freqs, mags, resolution, bpo):
    """pitch_tuning behind estimate_tuning's median threshold, by numpy.median and numpy.histogram on the header's edges."""
    f = np.asarray(freqs, np.float32)
    keep = f > 0
    f = f[keep]
    if not f.size:
        return 0.0, 0, 0
    n = f.size
    if mags is not None:
        m = np.asarray(mags, np.float32)[keep]
        f = f[m >= np.median(m)]
    e = tm.edges(resolution)
    counts, _ = np.histogram(tm.residuals(f, bpo), bins=e)
    return float(e[np.argmax(counts)]), int(n), int(f.size)


def seeded_cases():
    rng = np.random.default_rng(5)
    cases = {}
    f = (27.5 * 2.0 ** (rng.uniform(2.0, 7.0, 4001))).astype(np.float32)
    f[rng.random(f.size) < 0.3] = 0.0
    cases["random_odd"] = (f, rng.random(f.size).astype(np.float32))
    cases["random_even"] = (f[:-1], rng.random(f.size - 1).astype(np.float32))
    det = (440.0 * 2.0 ** ((rng.integers(-24, 24, 600) + 0.23 + 0.02 * rng.standard_normal(600)) / 12.0)).astype(np.float32)
    cases["detuned"] = (det, (1.0 + rng.random(600)).astype(np.float32))
    cases["empty"] = (np.zeros(0, np.float32), np.zeros(0, np.float32))
    cases["all_zero_pitch"] = (np.zeros(7, np.float32), np.ones(7, np.float32))
    cases["one"] = (np.array([445.0], np.float32), np.array([2.0], np.float32))
    cases["two"] = (np.array([445.0, 452.0], np.float32), np.array([2.0, 3.0], np.float32))
    cases["even_middles_differ"] = (np.array([441.0, 445.0, 452.0, 460.0], np.float32), np.array([1.0, 2.0, 4.0, 8.0], np.float32))
    cases["equal_mags"] = (det[:101], np.full(101, 0.5, np.float32))
    cases["below_27_5"] = (np.array([10.0, 13.0, 20.0, 443.0], np.float32), np.ones(4, np.float32))
    return cases


@pytest.mark.parametrize("resolution", [0.01, 0.3, 1.0 / 4096.0])
@pytest.mark.parametrize("bpo", [12, 36])
def test_pitch_tuning_against_the_model_and_numpy(lib, resolution, bpo):
    for name, (f, m) in seeded_cases().items():
        for mags in (m, None):
            got = binding.pitch_tuning(f, mags, resolution, bpo)
            want = tm.pitch_tuning(f, mags, resolution, bpo)
            assert want["admitted"] == [want["tuning"]], (name, "a residual of a seeded case sits on an edge")
            assert got == (want["tuning"], want["n"], want["selected"]), (name, mags is None, got, want)
            assert got == numpy_tuning(f, mags, resolution, bpo), (name, mags is None)
    # the middles of an even count differ: the threshold is their float32 mean, 3.0, and two entries pass it
    f, m = seeded_cases()["even_middles_differ"]
    assert binding.pitch_tuning(f, m, resolution, bpo)[1:] == (4, 2)
    assert binding.pitch_tuning(f[:1], m[:1], resolution, bpo)[1:] == (1, 1) and binding.pitch_tuning(f[:2], m[:2], resolution, bpo)[1:] == (2, 1)
    assert binding.pitch_tuning(f[:0], m[:0], resolution, bpo) == (0.0, 0, 0)


def test_a_residual_on_an_edge_and_a_tie(lib):
    """pitch = 27.5 * 2^j has residual 0.0 exactly, the edge e_50 of resolution 0.01: it counts in bin 50 ([0, 0.01)), not in 49. Two
    bins with the same largest count: the first wins."""
    on_edge = np.array([27.5 * 2 ** j for j in range(1, 6)], np.float32)
    assert (tm.residuals(on_edge) == 0.0).all()
    assert binding.pitch_tuning(on_edge)[0] == tm.edges(0.01)[50] == tm.pitch_tuning(on_edge)["tuning"]
    e = tm.edges(0.01)
    lo_bin, hi_bin = 20, 70  # residual centres -0.295 and 0.205
    f = lambda b, octave: 27.5 * 2.0 ** (octave + (e[b] + 0.005) / 12.0)
    tie = np.array([f(hi_bin, 3), f(hi_bin, 4), f(lo_bin, 3), f(lo_bin, 5), f(40, 4)], np.float32)
    want = tm.pitch_tuning(tie)
    assert want["tuning"] == e[lo_bin] and want["admitted"] == [e[lo_bin]]
    assert binding.pitch_tuning(tie) == (e[lo_bin], 5, 5)
    assert binding.pitch_tuning(tie[::-1].copy()) == (e[lo_bin], 5, 5)


def test_piptrack_bins_where_fmax_clips_to_nyquist(lib):
    from parseoggvorbis_amd import tuning
    for n_fft in (64, 1102, 2048):
        spec = tuning.framing_spec(n_fft)
        for sr in (4000, 7999, 8000, 11025, 22050, 44100):
            for fmin, fmax in ((150.0, 4000.0), (0.0, 1e9), (-5.0, 200.0), (3999.0, 4000.0), (150.0, 150.0 + 1e-9)):
                tun = tuning.tuning_spec(fmin, fmax)
                got = binding.piptrack_bins(sr, spec, tun)
                assert got == tm.bins(sr, n_fft, fmin, fmax), (n_fft, sr, fmin, fmax, got)
                if fmax >= sr / 2.0 and fmin <= 0.0:  # the whole band but the Nyquist bin itself: k sr / n_fft < sr / 2
                    assert got == (0, n_fft // 2)
    out = np.zeros(2, np.uint32)
    assert lib.vsyn_piptrack_bins(0, C.byref(spec), C.byref(tun), out.ctypes.data) == binding.VSYN_ERR_INVALID
    assert lib.vsyn_piptrack_bins(8000, C.byref(spec), C.byref(tun), None) == binding.VSYN_ERR_INVALID


def test_the_vectorised_piptrack_is_the_plain_loop():
    rng = np.random.default_rng(11)
    for n_fft, sr in ((64, 8000), (127, 22050)):
        nb = n_fft // 2 + 1
        S = (rng.random((9, nb)) ** 4).astype(np.float32)
        S[1] = 0.0                      # a silent frame: no peak
        S[2, 5:9] = S[2, 5]             # a plateau: its first bin fails >, the next are no peaks either but the last before a drop
        S[3, -1] = 10.0                 # the last bin is the frame's maximum
        S[4, 0] = 10.0                  # bin 0 never is a peak
        S[5, 7] = np.nan                # a frame that is not finite
        S[6, 3] = np.inf
        S[7] = np.float32(1e-42)        # denormal plateau: b = 0 gets + 1
        for fmin, fmax, thr in ((0.0, 1e9, 0.1), (150.0, 4000.0, 0.1), (150.0, 4000.0, 0.0), (0.0, 1e9, 0.9)):
            p, m = tm.piptrack(S, sr, n_fft, fmin, fmax, thr)
            pl, ml = tm.piptrack_loop(S, sr, n_fft, fmin, fmax, thr)
            assert np.array_equal(p, pl, equal_nan=True) and np.array_equal(m, ml, equal_nan=True), (n_fft, fmin, fmax, thr)
            assert np.isnan(p[5]).all() and np.isnan(m[6]).all() and not p[1].any() and p[4, 0] == 0
        p, _ = tm.piptrack(S, sr, n_fft, 0.0, 1e9, 0.1)
        # the last bin can be a peak, at its own frequency, where it lies below sr / 2: for an odd n_fft alone (fmax' <= sr / 2)
        assert p[3, -1] == (np.float32((nb - 1) * sr / n_fft) if n_fft % 2 else 0)


BAD_TUNING = [(dict(fmin=float("nan")), "fmin"), (dict(fmax=float("inf")), "fmax"), (dict(fmin=300.0, fmax=300.0), "fmax"),
              (dict(fmin=-10.0, fmax=0.0), "fmax"), (dict(threshold=-0.1), "threshold"), (dict(threshold=float("nan")), "threshold"),
              (dict(resolution=0.0), "resolution"), (dict(resolution=1.0), "resolution"), (dict(resolution=float("nan")), "resolution"),
              (dict(resolution=1.0 / 4097.0), "resolution"), (dict(bins_per_octave=0), "bins_per_octave"),
              (dict(bins_per_octave=257), "bins_per_octave")]


def _c_tuning(**kw):
    d = dict(tm.DEFAULTS, **kw)
    return binding.TuningSpec(d["fmin"], d["fmax"], d["threshold"], d["resolution"], d["bins_per_octave"], d.get("reserved", 0))


@pytest.mark.parametrize("kw,name", BAD_TUNING + [(dict(reserved=1), "reserved")])
def test_refusals_from_c(lib, kw, name):
    from parseoggvorbis_amd import spectral
    spec = spectral.spectral_spec("lin_power", n_fft=2048, hop_length=512, power=1)
    err = C.c_char_p()
    assert lib.vsyn_tuning_check(C.byref(spec), C.byref(_c_tuning()), C.byref(err)) == binding.VSYN_OK
    assert lib.vsyn_tuning_check(C.byref(spec), C.byref(_c_tuning(**kw)), C.byref(err)) == binding.VSYN_ERR_INVALID
    assert name.encode() in err.value, err.value
    out = np.zeros(2, np.uint32)
    assert lib.vsyn_piptrack_bins(22050, C.byref(spec), C.byref(_c_tuning(**kw)), out.ctypes.data) == binding.VSYN_ERR_INVALID
    if name in ("resolution", "bins_per_octave"):
        d = dict(tm.DEFAULTS, **kw)
        t, cnt, f = np.full(1, 7.0), np.full(2, 9, np.uint64), np.array([440.0], np.float32)
        assert lib.vsyn_pitch_tuning(f.ctypes.data, None, 1, d["resolution"], d["bins_per_octave"], t.ctypes.data, cnt.ctypes.data) == binding.VSYN_ERR_INVALID
        assert t[0] == 7.0 and (cnt == 9).all()  # nothing written


def test_the_spectral_spec_is_checked_as_for_the_linear_spectra(lib):
    from parseoggvorbis_amd import spectral
    err = C.c_char_p()
    tun = _c_tuning()
    for kind in ("lin_db", "stft", "log_mel", "chroma"):
        spec = spectral.spectral_spec(kind, n_fft=512, hop_length=128)
        assert lib.vsyn_tuning_check(C.byref(spec), C.byref(tun), C.byref(err)) == binding.VSYN_ERR_INVALID and b"lin_power" in err.value
        assert lib.vsyn_piptrack_tile(C.byref(spec)) == 0
    for field, value, name in (("n_fft", 8, b"n_fft"), ("hop_length", 0, b"hop_length"), ("win_length", 0, b"win_length"), ("power", 3, b"power"),
                               ("options", 8, b"options")):
        spec = spectral.spectral_spec("lin_power", n_fft=512, hop_length=128)
        setattr(spec, field, value)
        assert lib.vsyn_tuning_check(C.byref(spec), C.byref(tun), C.byref(err)) == binding.VSYN_ERR_INVALID and name in err.value
    assert lib.vsyn_tuning_check(C.byref(spec), None, C.byref(err)) == binding.VSYN_ERR_INVALID
    ok = spectral.spectral_spec("lin_power", n_fft=512, hop_length=128)
    assert lib.vsyn_tuning_check(C.byref(ok), None, C.byref(err)) == binding.VSYN_ERR_INVALID and b"NULL" in err.value
    # the device entries refuse the same before they touch a device (the handle is looked at first: no device is needed to say so)
    assert lib.vsyn_tuning_device(None, C.byref(ok), C.byref(tun), 0, None, None, 0, 1, None, None, None, None, C.byref(err)) == binding.VSYN_ERR_INVALID
    assert b"handle" in err.value
    # the tile of the tests: the FFT kernel's for a power of two, the direct kernel's otherwise
    assert [lib.vsyn_piptrack_tile(C.byref(spectral.spectral_spec("lin_power", n_fft=n, hop_length=h, power=1)))
            for n, h in ((2048, 512), (512, 128), (64, 16), (1102, 441), (8191, 1))] == [1, 4, 32, 8, 1]


def test_refusals_in_python_before_the_library_loads():
    code = r"""
import sys
from parseoggvorbis_amd import tuning
bad = [dict(fmin=float("nan")), dict(fmax=float("inf")), dict(fmin=300.0, fmax=300.0), dict(fmin=-10.0, fmax=0.0), dict(threshold=-0.1),
       dict(threshold=float("nan")), dict(resolution=0.0), dict(resolution=1.0), dict(resolution=1.0 / 4097.0), dict(resolution="0.01"),
       dict(bins_per_octave=0), dict(bins_per_octave=257), dict(bins_per_octave=12.0), dict(fmin=True)]
for kw in bad:
    try:
        tuning.tuning_spec(**kw)
    except tuning.TuningError as e:
        assert list(kw)[-1] in str(e), (kw, str(e))
    else:
        raise SystemExit("accepted: %r" % (kw,))
for kw in (dict(n_fft=8), dict(n_fft=2048, hop_length=0), dict(power=3), dict(win_length=4096), dict(center=1), dict(n_fft=2048.0)):
    for fn in (tuning.get_tuning_batch, tuning.get_piptrack_batch):
        try:
            fn([b"x"], **kw)
        except tuning.TuningError:
            pass
        else:
            raise SystemExit("accepted: %r" % (kw,))
for kw in (dict(errors="ignore"), dict(sr=0), dict(threads=-1), dict(files_per_submit=0)):
    try:
        tuning.get_tuning_batch([b"x"], **kw)
    except tuning.TuningError:
        pass
    else:
        raise SystemExit("accepted: %r" % (kw,))
s = tuning.framing_spec(1024)
assert (s.hop_length, s.win_length, s.power, s.kind) == (256, 1024, 1, 5)
t = tuning.tuning_spec()
assert (t.fmin, t.fmax, t.threshold, t.resolution, t.bins_per_octave, t.reserved) == (150.0, 4000.0, 0.1, 0.01, 12, 0)
from parseoggvorbis_amd import binding, _corpus
assert binding._lib is None and _corpus._lib is None, "a library was loaded"
print("ok")
"""
    import subprocess
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=entry.ROOT)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


def test_tuning_estimate_is_accepted_where_the_library_is_not_needed():
    code = r"""
import inspect
from parseoggvorbis_amd import cqt, rhythm, spectral
a = {k: p.default for k, p in inspect.signature(spectral.get_spectral_batch).parameters.items()}
a.update(list_of_bytes=[], kind="tonnetz", tuning="estimate", n_chroma=24, tuning_resolution=0.02, tuning_fmin=100.0, tuning_fmax=3000.0,
         tuning_threshold=0.2)
c = spectral.checked_specs(a)
e = c.est
assert (e.fmin, e.fmax, e.threshold, e.resolution, e.bins_per_octave) == (100.0, 3000.0, 0.2, 0.02, 24) and c.chroma.tuning == 0.0
assert spectral.checked_specs(dict(a, tuning=0.25)).est is None
for kw, word in ((dict(kind="log_mel"), "chroma"), (dict(tuning_resolution=0.0), "tuning_resolution"), (dict(tuning_fmax=50.0), "tuning_fmax"),
                 (dict(tuning_threshold=-1.0), "tuning_threshold"), (dict(tuning_fmin=float("nan")), "tuning_fmin"), (dict(tuning=None), "tuning"),
                 (dict(tuning="a"), "tuning"), (dict(tuning="Estimate"), "tuning")):
    try:
        spectral.checked_specs(dict(a, **kw))
    except spectral.SpectralError as ex:
        assert word in str(ex), (kw, str(ex))
    else:
        raise SystemExit("accepted: %r" % (kw,))
b = dict(a)
del b["tuning_resolution"]
try:
    spectral.checked_specs(b)  # the rhythm entries forward the same arguments and have no estimate
except spectral.SpectralError as ex:
    assert "get_spectral_batch" in str(ex)
else:
    raise SystemExit("accepted without the estimator's arguments")
t, e = cqt._estimate("estimate", 36, 0.01, 150.0, 4000.0, 0.1)
assert t == 0.0 and e.bins_per_octave == 36 and cqt._estimate(0.25, 36, 0.01, 150.0, 4000.0, 0.1) == (0.25, None)
for fn, kw in ((cqt.get_cqt_batch, dict(tuning_resolution=1.0)), (cqt.get_chroma_cqt_batch, dict(tuning_fmax=-1.0)), (cqt.get_cqt_batch, dict(tuning=None))):
    try:
        fn([b"x"], **dict(dict(tuning="estimate"), **kw))
    except cqt.CqtError:
        pass
    else:
        raise SystemExit("accepted: %r" % (kw,))
from parseoggvorbis_amd import binding, _corpus
assert binding._lib is None and _corpus._lib is None, "a library was loaded"
print("ok")
"""
    import subprocess
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=entry.ROOT)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


# ---- what the GPU tests rely on ----

def test_the_models_tiles_are_the_librarys(lib):
    from parseoggvorbis_amd import tuning
    for (n, hop, win, center), tile in tm.GRID_TILES.items():
        assert lib.vsyn_piptrack_tile(C.byref(tuning.framing_spec(n, hop, win, center))) == tile


@pytest.mark.parametrize("framing", tm.GRID, ids=tm.grid_id)
def test_the_chords_decision_bands_stay_under_the_cap(framing):
    """With the real band S +- dS of the linear spectra's bound, at most 1 % of the model's peaks are undecided, at every framing and
    both powers, on the very segments the GPU test runs (frame counts 1, tile - 1, tile, tile + 1, 2 tile + 1); and the chord has
    peaks to decide."""
    n, hop, win, center = framing
    for power in (1, 2):
        peaks = undecided = 0
        for y in tm.grid_segments(framing):
            X, B = lm.stft(y, n, hop, win, center)
            S, dS = lm.power_bound(X, B, power)
            D = tm.decisions(S, dS, tm.GRID_SR, n)
            model = tm.piptrack(S.astype(np.float32), tm.GRID_SR, n)[0] > 0
            peaks += int(model.sum())
            undecided += int((model & ~D["peak"] & ~D["nonpeak"]).sum())
            assert not (model & D["nonpeak"]).any() and not (~model & D["peak"]).any()  # the model itself lies inside its band
        assert peaks >= 20 and undecided <= 0.01 * peaks, (framing, power, peaks, undecided)


def test_no_residual_of_the_chord_sits_on_an_edge():
    """The exception of the exact comparison (a selected residual within 1e-9 of an edge whose bin competes for the arg-max) does not
    occur for the chord cases, and at n_fft 2048 the estimate finds the detune to within the histogram's bin and the interpolation's
    bias (0.49 is half a bin from wrapping: the distance is taken around the circle)."""
    for n, hop, win, center in tm.GRID:
        for i, det in enumerate((0.23, -0.37, 0.0, 0.49)):
            y = tm.chord(22050, tm.GRID_SR, det, seed=i)
            X, _ = lm.stft(y, n, hop, win, center)
            p, m = tm.piptrack(np.abs(X).astype(np.float32), tm.GRID_SR, n)
            r = tm.pitch_tuning(p, m)
            assert r["admitted"] == [r["tuning"]] and r["n"] > 0, (n, det, r)
            if n == 2048:
                d = abs(r["tuning"] + 0.005 - det)
                assert min(d, 1.0 - d) <= 0.03, (det, r["tuning"])
