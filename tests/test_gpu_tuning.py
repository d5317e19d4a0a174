"""Tuning estimation on the GPU (include/vorbis_synth_hip.h, "tuning estimation"; model and bounds: tests/tuning_model.py).

  1. The dense piptrack rows against the float64 model with decision bands: zeros at decided non-peaks, pitch and mag within the
     derived bounds at decided peaks, either outcome where the band of the linear spectra's bound cannot decide; at most 1 % of the
     model's peaks are undecided (rehearsed on the CPU, tests/test_tuning_cpu.py). And the rows are the float32 model on the device's
     own lin_power rows, bit for bit: the spectrum the peaks are picked from is that kind's.
  2. The reduction, exactly: vsyn_tuning_device's double and counts equal the model's reduction of the device's own rows.
  3. Independence of slot and batch, a NaN sample, the host entry on the last submit's PCM, and the corpus entries end to end.
  4. tuning="estimate": the rows of the estimate entries (chroma, tonnetz, cqt, chroma_cqt) equal, bit for bit, the rows of the existing
     entries called with the returned tuning, segment by segment, with several tunings and two rates in one call; the returned
     tuning is the tuning stage's at the matching parameters. Through Synth on a submit's PCM and end to end on Ogg files.
"""
import ctypes as C

import numpy as np
import pytest

from tests import spectral_lin_model as lm
from tests import spectral_model as sm
from tests import tuning_model as tm

pytestmark = pytest.mark.gpu

SR = tm.GRID_SR


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from parseoggvorbis_amd import spectral, tuning
    return spectral, tuning


@pytest.fixture(scope="module")
def synth():
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    yield g
    g.close()


def batch(signals, channels=1):
    plane = max(max(len(y) for y in signals), 1)
    pcm = np.zeros((len(signals), channels, plane), np.float32)
    for i, y in enumerate(signals):
        pcm[i, :, :len(y)] = y
    return pcm, [len(y) for y in signals]


def upload(pcm, frames):
    import torch
    return torch.from_numpy(np.ascontiguousarray(pcm, np.float32)).cuda(), torch.from_numpy(np.asarray(frames, np.int32)).cuda()


def run_piptrack(g, spec, tun, pcm, frames, rates):
    """vsyn_piptrack_device: the list of each segment's (pitch, mag), float32 [F_g][NB]; nothing is written past the rows."""
    import torch
    S, Cn, plane = pcm.shape
    nb = spec.n_fft // 2 + 1
    fmax = sm.num_frames(plane, spec.n_fft, spec.hop_length, bool(spec.options & 1))
    d_pcm, d_frames = upload(pcm, frames)
    d_p = torch.full((S * fmax + 1, nb), float("nan"), dtype=torch.float32, device="cuda")
    d_m = torch.full((S * fmax + 1, nb), float("nan"), dtype=torch.float32, device="cuda")
    d_off = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    g.piptrack_device(spec, tun, rates, d_pcm.data_ptr(), plane, Cn, d_frames.data_ptr(), d_p.data_ptr(), d_m.data_ptr(), d_off.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    off, p, m = d_off.cpu().numpy(), d_p.cpu().numpy(), d_m.cpu().numpy()
    assert off[0] == 0 and off[S] <= S * fmax
    assert np.isnan(p[off[S]:]).all() and np.isnan(m[off[S]:]).all()
    return [(p[off[i]:off[i + 1]], m[off[i]:off[i + 1]]) for i in range(S)]


def run_tuning(g, spec, tun, pcm, frames, rates):
    """vsyn_tuning_device: (tuning float64 [S], counts uint64 [S][2])."""
    import torch
    S, Cn, plane = pcm.shape
    d_pcm, d_frames = upload(pcm, frames)
    d_t = torch.full((S + 1,), float("nan"), dtype=torch.float64, device="cuda")
    d_c = torch.full((S + 1, 2), -1, dtype=torch.int64, device="cuda")
    g.tuning_device(spec, tun, rates, d_pcm.data_ptr(), plane, Cn, d_frames.data_ptr(), d_t.data_ptr(), d_c.data_ptr(),
                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    t, c = d_t.cpu().numpy(), d_c.cpu().numpy()
    assert np.isnan(t[S]) and (c[S] == -1).all()
    return t[:S], c[:S].astype(np.uint64)


def run_lin_power(g, spec, pcm, frames, rates):
    import torch
    S, Cn, plane = pcm.shape
    nb = spec.n_fft // 2 + 1
    fmax = sm.num_frames(plane, spec.n_fft, spec.hop_length, bool(spec.options & 1))
    d_pcm, d_frames = upload(pcm, frames)
    d_rows = torch.zeros((S * fmax + 1, nb), dtype=torch.float32, device="cuda")
    d_off = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    g.spectral_device(spec, rates, d_pcm.data_ptr(), plane, Cn, d_frames.data_ptr(), d_rows.data_ptr(), d_off.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    off, rows = d_off.cpu().numpy(), d_rows.cpu().numpy()
    return [rows[off[i]:off[i + 1]] for i in range(S)]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. the rows ----

@pytest.mark.parametrize("framing", tm.GRID, ids=tm.grid_id)
def test_piptrack_rows_against_the_model_with_decision_bands(mods, synth, framing):
    _, tuning = mods
    n, hop, win, center = framing
    tile = synth.lib.vsyn_piptrack_tile(C.byref(tuning.framing_spec(n, hop, win, center)))
    assert tile == tm.GRID_TILES[framing]
    sigs = tm.grid_segments(framing)
    pcm, frames = batch(sigs)
    tun = tuning.tuning_spec()
    for power in (1, 2):
        spec = tuning.framing_spec(n, hop, win, center, power)
        rows = run_piptrack(synth, spec, tun, pcm, frames, [SR] * len(sigs))
        lin = run_lin_power(synth, spec, pcm, frames, [SR] * len(sigs))
        peaks = undecided = 0
        worst = 0.0
        for y, (p, m), S_dev in zip(sigs, rows, lin):
            assert p.shape[0] == sm.num_frames(len(y), n, hop, center) > 0
            X, B = lm.stft(y, n, hop, win, center)
            S, dS = lm.power_bound(X, B, power)
            D = tm.decisions(S, dS, SR, n)
            u, e = tm.check_rows(p, m, D, what=(framing, power, len(y)))
            worst = max(worst, e)
            model = tm.piptrack(S.astype(np.float32), SR, n)[0] > 0
            peaks += int(model.sum())
            undecided += int((model & ~D["peak"] & ~D["nonpeak"]).sum())
            wp, wm = tm.piptrack(S_dev, SR, n)  # the float32 arithmetic on the device's own spectrum: the same bits
            assert same_bits(p, wp) and same_bits(m, wm), (framing, power, len(y))
        print("%s power %d: %d model peaks, %d undecided, worst |d| / bound %.3f" % (tm.grid_id(framing), power, peaks, undecided, worst))
        assert peaks >= 20 and undecided <= 0.01 * peaks, (framing, power, peaks, undecided)


def test_the_band_the_threshold_and_an_odd_n_fft(mods, synth):
    """fmin / fmax other than the defaults, a threshold of 0 (every local maximum of the band) and of 0.9, a rate whose Nyquist clips
    fmax, and n_fft = 127, where the last bin lies inside the band and can be a peak: the float32 model on the device's own
    spectrum, bit for bit."""
    _, tuning = mods
    rng = np.random.default_rng(2)
    y = tm.chord(3000, 8000, 0.1, seed=3, noise=1e-2)
    hi = (y + 0.2 * np.sin(np.pi * (1.0 - 1.0 / 127.0) * np.arange(3000))).astype(np.float32)  # a partial at the last bin of n_fft 127
    pcm, frames = batch([y, hi, (0.1 * rng.standard_normal(1500)).astype(np.float32)])
    for n, hop in ((256, 64), (127, 50)):
        spec = tuning.framing_spec(n, hop)
        lin = run_lin_power(synth, spec, pcm, frames, [8000] * 3)
        for kw in (dict(), dict(fmin=0.0, fmax=1e6), dict(fmin=400.0, fmax=900.0), dict(threshold=0.0), dict(threshold=0.9, fmin=-3.0)):
            tun = tuning.tuning_spec(**kw)
            rows = run_piptrack(synth, spec, tun, pcm, frames, [8000] * 3)
            d = dict(tm.DEFAULTS, **kw)
            last = 0
            for (p, m), S_dev in zip(rows, lin):
                wp, wm = tm.piptrack(S_dev, 8000, n, d["fmin"], d["fmax"], d["threshold"])
                assert same_bits(p, wp) and same_bits(m, wm) and (kw.get("threshold") == 0.9 or (wp > 0).sum() > 0), (n, kw)
                last += int((p[:, -1] > 0).sum())
            if n == 127 and kw.get("fmax") == 1e6:
                assert last > 0  # the last bin was a peak somewhere


# ---- 2. the reduction ----

@pytest.mark.parametrize("framing", [tm.GRID[0], tm.GRID[1], tm.GRID[3]], ids=tm.grid_id)
def test_the_reduction_is_the_models_on_the_devices_rows(mods, synth, framing):
    _, tuning = mods
    n, hop, win, center = framing
    T = 9000
    sig = lm.signals(T, n)
    names = ["chord", "chord_flat"] + sorted(sig) + ["zero", "short"]
    sigs = [tm.chord(T, SR, 0.23, seed=1), tm.chord(T - 700, SR, -0.37, seed=2)] + [sig[k] for k in sorted(sig)] + \
           [np.zeros(T // 2, np.float32), tm.chord(3, SR, 0.0)]
    pcm, frames = batch(sigs)
    rates = [SR] * len(sigs)
    for kw in (dict(), dict(resolution=0.3, bins_per_octave=36), dict(resolution=1.0 / 4096.0, fmin=0.0, fmax=1e6, threshold=0.0)):
        tun = tuning.tuning_spec(**kw)
        d = dict(tm.DEFAULTS, **kw)
        for power in (1, 2):
            spec = tuning.framing_spec(n, hop, win, center, power)
            rows = run_piptrack(synth, spec, tun, pcm, frames, rates)
            t, c = run_tuning(synth, spec, tun, pcm, frames, rates)
            for i, name in enumerate(names):
                want = tm.pitch_tuning(rows[i][0], rows[i][1], d["resolution"], d["bins_per_octave"])
                assert (int(c[i, 0]), int(c[i, 1])) == (want["n"], want["selected"]), (framing, kw, power, name, c[i], want)
                assert t[i] in want["admitted"], (framing, kw, power, name, t[i], want)
                if name in ("chord", "chord_flat") and not kw:
                    assert want["admitted"] == [want["tuning"]] and want["n"] > 50
                if name == "zero":
                    assert t[i] == 0.0 and want["n"] == 0
            if not kw and n == 2048 and power == 1:  # and the estimate means something: the chords' detunes, to a bin and the bias
                assert abs(t[0] + 0.005 - 0.23) <= 0.03 and abs(t[1] + 0.005 + 0.37) <= 0.03, t[:2]


def test_two_rates_and_a_skipped_segment(mods, synth):
    """The same samples at two rates: the band's bins and the pitches differ by the rate, so do the tunings; a rate of 0 gives no rows,
    tuning 0.0 and counts 0; stereo is the float32 downmix of the linear spectra."""
    _, tuning = mods
    y = tm.chord(6000, SR, 0.23, seed=4)
    pcm, frames = batch([y, y, y, y[:4000]], channels=2)
    pcm[:, 1] *= 0.5
    rates = [SR, 16000, 0, 16000]
    spec, tun = tuning.framing_spec(1024, 256), tuning.tuning_spec()
    rows = run_piptrack(synth, spec, tun, pcm, frames, rates)
    lin = run_lin_power(synth, spec, pcm, frames, rates)
    t, c = run_tuning(synth, spec, tun, pcm, frames, rates)
    assert rows[2][0].shape[0] == 0 and t[2] == 0.0 and (c[2] == 0).all()
    for i in (0, 1, 3):
        wp, wm = tm.piptrack(lin[i], rates[i], 1024)
        assert same_bits(rows[i][0], wp) and same_bits(rows[i][1], wm)
        want = tm.pitch_tuning(wp, wm)
        assert t[i] in want["admitted"] and (int(c[i, 0]), int(c[i, 1])) == (want["n"], want["selected"]) and want["n"] > 0
    assert not same_bits(rows[0][0], rows[1][0])


# ---- 3. independence, non-finite samples, the host entries ----

@pytest.mark.parametrize("framing", [tm.GRID[1], tm.GRID[3]], ids=tm.grid_id)
def test_same_bits_alone_and_in_a_batch_and_one_nan_sample(mods, synth, framing):
    _, tuning = mods
    n, hop, win, center = framing
    spec, tun = tuning.framing_spec(n, hop, None, center), tuning.tuning_spec()
    T = 11 * hop + n
    y = tm.chord(T, SR, 0.23, seed=5)
    alone_p, alone_m = run_piptrack(synth, spec, tun, y[None, None, :], [T], [SR])[0]
    alone_t, alone_c = run_tuning(synth, spec, tun, y[None, None, :], [T], [SR])
    assert np.isfinite(alone_p).all() and alone_c[0, 0] > 0
    pcm, frames = batch([tm.chord(T + 3 * hop + 1, SR, -0.4, seed=6), y, tm.chord(T - 2 * hop - 5, SR, 0.1, seed=7)])
    rows = run_piptrack(synth, spec, tun, pcm, frames, [SR] * 3)
    t, c = run_tuning(synth, spec, tun, pcm, frames, [SR] * 3)
    assert same_bits(rows[1][0], alone_p) and same_bits(rows[1][1], alone_m) and t[1] == alone_t[0] and (c[1] == alone_c[0]).all()
    # one NaN sample: exactly the frames that contain it are NaN, the others keep their bits, and only their peaks leave the tuning
    bad = y.copy()
    at = 5 * hop + 7
    bad[at] = np.nan
    pad = n // 2 if center else 0
    F = alone_p.shape[0]
    hit = np.array([f * hop - pad <= at < f * hop - pad + n for f in range(F)])
    assert 0 < hit.sum() < F
    p, m = run_piptrack(synth, spec, tun, bad[None, None, :], [T], [SR])[0]
    assert np.isnan(p[hit]).all() and np.isnan(m[hit]).all()
    assert same_bits(p[~hit], alone_p[~hit]) and same_bits(m[~hit], alone_m[~hit])
    tb, cb = run_tuning(synth, spec, tun, bad[None, None, :], [T], [SR])
    want = tm.pitch_tuning(alone_p[~hit], alone_m[~hit])
    assert tb[0] in want["admitted"] and (int(cb[0, 0]), int(cb[0, 1])) == (want["n"], want["selected"])
    assert int(cb[0, 0]) == int(alone_c[0, 0]) - int((alone_p[hit] > 0).sum())


def test_the_host_entry_on_the_last_submits_pcm(mods):
    """vsyn_pcm_tuning_host, tuning only and with the rows, at the PCM's own rate and behind the resampler: what the device entries give
    on the PCM that vsyn_pcm_fetch_host / vsyn_pcm_resample_host return, and the next submit is not disturbed."""
    _, tuning = mods
    from parseoggvorbis_amd.binding import Synth, VSYN_PCM_F32
    from tests.workloads import fixture_like_spec, synth_batch
    setup = fixture_like_spec(2)
    b = synth_batch(setup, streams=3, packets_per_stream=14, pattern="mixed", seed=21)
    S = len(b["segments"])
    g = Synth(setup, device=0, max_streams=4)
    assert g.submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"], flags=4)["rc"] == 0  # KEEP_PCM
    pcm, fr = g.pcm_fetch_host(VSYN_PCM_F32, S, b["plane_stride"])
    pcm = np.ascontiguousarray(pcm.transpose(0, 2, 1))  # [S][C][plane]
    spec, tun = tuning.framing_spec(512, 128, power=2), tuning.tuning_spec(threshold=0.05)
    rates = [44100, 22050, 44100][:S] + [44100] * max(0, S - 3)
    only = g.pcm_tuning_host(spec, tun, rates)
    full = g.pcm_tuning_host(spec, tun, rates, rows=True)
    assert only["rc"] == 0 and full["rc"] == 0 and np.array_equal(only["tuning"], full["tuning"]) and np.array_equal(only["counts"], full["counts"])
    assert np.array_equal(only["seg_rows"], full["seg_rows"]) and full["pitches"].shape == (int(full["seg_rows"].sum()), 257)
    rows = run_piptrack(g, spec, tun, pcm, [int(f) for f in fr], rates)
    t, c = run_tuning(g, spec, tun, pcm, [int(f) for f in fr], rates)
    o = 0
    for i in range(S):
        nr = int(full["seg_rows"][i])
        assert nr == rows[i][0].shape[0] > 0
        assert same_bits(full["pitches"][o:o + nr], rows[i][0]) and same_bits(full["mags"][o:o + nr], rows[i][1])
        o += nr
    assert np.array_equal(t, full["tuning"]) and np.array_equal(c, full["counts"]) and full["counts"][:, 0].sum() > 0
    res = g.pcm_tuning_host(spec, tun, rates, out_rate=16000, rows=True)
    rp, rf = g.pcm_resample_host(rates, 16000)
    want = run_piptrack(g, spec, tun, rp, [int(f) for f in rf], [16000] * S)
    assert same_bits(res["pitches"], np.concatenate([w[0] for w in want])) and same_bits(res["mags"], np.concatenate([w[1] for w in want]))
    again = g.submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"])
    assert again["rc"] == 0
    g.close()


# ---- end to end through the corpus entries ----

E2E_FILES = ["test.mono44khz", "test.stereo44khz", "synth_04"]


@pytest.mark.parametrize("sr", [None, 16000])
def test_end_to_end_on_ogg_files(mods, sr):
    """get_piptrack_batch is the float32 model on get_spectral_batch(kind="lin_power") at the same framing, bit for bit;
    get_tuning_batch is the model's reduction of those rows, with its counts; a file alone gives what it gives in the batch."""
    spectral, tuning = mods
    from tests.test_gpu_spectral import _ogg
    datas = [_ogg(n) for n in E2E_FILES]
    for kw in (dict(n_fft=2048, power=1), dict(n_fft=1102, hop_length=441, power=2, threshold=0.05, resolution=0.02, bins_per_octave=24)):
        fr = {k: v for k, v in kw.items() if k in ("n_fft", "hop_length", "power")}
        pk = {k: v for k, v in kw.items() if k not in ("resolution", "bins_per_octave")}
        hop = kw.get("hop_length", kw["n_fft"] // 4)
        lin = spectral.get_spectral_batch(datas, kind="lin_power", sr=sr, **dict(fr, hop_length=hop))
        rows = tuning.get_piptrack_batch(datas, sr=sr, **pk)
        counts = []
        tun = tuning.get_tuning_batch(datas, sr=sr, counts=counts, **kw)
        for i, (S_dev, (p, m, rate), (t, rate2)) in enumerate(zip(lin, rows, tun)):
            assert rate == rate2 == (sr or 44100) and p.shape == S_dev.shape and p.shape[0] > 0
            wp, wm = tm.piptrack(S_dev, rate, kw["n_fft"], threshold=kw.get("threshold", 0.1))
            assert same_bits(p, wp) and same_bits(m, wm), (kw, i)
            want = tm.pitch_tuning(p, m, kw.get("resolution", 0.01), kw.get("bins_per_octave", 12))
            assert t in want["admitted"] and counts[i] == (want["n"], want["selected"]), (kw, i, t, counts[i], want)
        assert sum(c[0] for c in counts[:2]) > 100  # the two recordings have peaks to estimate from (synth_04 may have none in the band)
        assert tuning.get_tuning_from_raw_bytes(datas[1], sr=sr, **kw) == tun[1]


def test_a_damaged_file_fails_alone(mods):
    _, tuning = mods
    from tests.test_gpu_spectral import _ogg
    blobs = [_ogg(n) for n in E2E_FILES]
    good = tuning.get_tuning_batch(blobs)
    bad = bytearray(blobs[1])
    bad[len(bad) // 2] ^= 0x55  # a page CRC
    res = tuning.get_tuning_batch([blobs[0], bytes(bad), blobs[2]], errors="return")
    assert isinstance(res[1], tuning.TuningError) and "file 1" in str(res[1])
    assert res[0] == good[0] and res[2] == good[2]
    with pytest.raises(tuning.TuningError):
        tuning.get_piptrack_batch([blobs[0], bytes(bad)])


# ---- tuning="estimate" ----

def test_a_call_that_could_hold_more_than_2_31_peaks_is_refused_by_name(mods, synth):
    """2^31 frames of n_fft 16 at hop 1 with four records a frame: refused before anything is allocated or launched."""
    import torch
    from parseoggvorbis_amd.binding import VSYN_ERR_INVALID, VsynError
    _, tuning = mods
    spec, tun = tuning.framing_spec(16, 1), tuning.tuning_spec(0.0, 1e9)
    d = torch.zeros(64, dtype=torch.float32, device="cuda")
    d_frames = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_t = torch.zeros(1, dtype=torch.float64, device="cuda")
    d_c = torch.zeros(2, dtype=torch.int64, device="cuda")
    with pytest.raises(VsynError) as ei:
        synth.tuning_device(spec, tun, [8000], d.data_ptr(), 1 << 31, 1, d_frames.data_ptr(), d_t.data_ptr(), d_c.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
    assert ei.value.code == VSYN_ERR_INVALID and "2^31 peaks" in str(ei.value)


@pytest.fixture(scope="module")
def submitted():
    """A handle whose last submit holds four stereo segments (a synthesis batch's PCM: broadband, each segment its own signal)."""
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec, synth_batch
    setup = fixture_like_spec(2)
    b = synth_batch(setup, streams=4, packets_per_stream=24, pattern="mixed", seed=31)
    g = Synth(setup, device=0, max_streams=4)
    assert g.submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"], flags=4)["rc"] == 0  # KEEP_PCM
    yield g, len(b["segments"])
    g.close()


def split_rows(r):
    o = np.concatenate([[0], np.cumsum(r["seg_rows"].astype(np.int64))])
    return [r["rows"][o[i]:o[i + 1]] for i in range(len(r["seg_rows"]))]


RATES = [22050, 22050, 16000, 22050]  # two tunings can meet at one rate, and a second rate: a bank index that is a rate index shows


@pytest.mark.parametrize("kind", ["chroma", "tonnetz"])
@pytest.mark.parametrize("out_rate", [0, 11025])
def test_chroma_estimate_equals_explicit_through_synth(mods, submitted, kind, out_rate):
    spectral, tuning = mods
    g, S = submitted
    rates = RATES[:S]
    for n_fft, hop, power, n_chroma in ((512, 128, 2, 12), (1102, 441, 1, 24)):
        spec = spectral.spectral_spec(kind, n_fft=n_fft, hop_length=hop, power=power)
        est = tuning.tuning_spec(threshold=0.05, bins_per_octave=n_chroma)
        got = g.pcm_chain_chroma_est_host(None, False, None, None, spec, spectral.chroma_spec(n_chroma=n_chroma, tuning=0.4), None, None, est, rates, out_rate)
        assert got["rc"] == 0
        t = got["tuning"]
        want_t = g.pcm_tuning_host(tuning.framing_spec(n_fft, hop, power=power), est, rates, out_rate)
        assert np.array_equal(t, want_t["tuning"]) and want_t["counts"][:, 0].min() > 0
        assert len(set(t.tolist())) > 1, t  # several tunings in one call
        rows = split_rows(got)
        for i in range(S):
            ref = g.pcm_chain_chroma_host(None, False, None, None, spec, spectral.chroma_spec(n_chroma=n_chroma, tuning=float(t[i])), None, None, rates, out_rate)
            assert rows[i].shape[0] > 0 and same_bits(rows[i], split_rows(ref)[i]), (kind, n_fft, i, t)
        # estimate = None is the existing entry, the struct's number used
        none = g.pcm_chain_chroma_est_host(None, False, None, None, spec, spectral.chroma_spec(n_chroma=n_chroma, tuning=float(t[0])), None, None, None, rates,
                                           out_rate)
        assert same_bits(split_rows(none)[0], rows[0]) and not none["tuning"].any()
    # behind the gate and conditioning: the estimate is taken from the signal the chroma kernel sees
    from parseoggvorbis_amd import pcm as pcm_mod
    spec = spectral.spectral_spec(kind, n_fft=512, hop_length=128)
    est = tuning.tuning_spec(threshold=0.05)
    cond, trim = pcm_mod.cond_spec(False, 0.97, spectral.SpectralError), pcm_mod.trim_spec(30.0, 512, 128, None, spectral.SpectralError)
    got = g.pcm_chain_chroma_est_host(trim, False, None, cond, spec, None, None, None, est, rates, out_rate)
    for i in range(S):
        ref = g.pcm_chain_chroma_host(trim, False, None, cond, spec, spectral.chroma_spec(tuning=float(got["tuning"][i])), None, None, rates, out_rate)
        assert same_bits(split_rows(got)[i], split_rows(ref)[i]) and np.array_equal(got["bounds"], ref["bounds"])


def test_chroma_estimate_refusals(mods, submitted):
    from parseoggvorbis_amd.binding import VsynError
    spectral, tuning = mods
    g, S = submitted
    rates = RATES[:S]
    chroma = spectral.spectral_spec("chroma", n_fft=512, hop_length=128)
    from parseoggvorbis_amd.binding import TuningSpec
    for spec, ch, est, word in ((spectral.spectral_spec("lin_power", n_fft=512, hop_length=128), None, tuning.tuning_spec(), "chroma kinds"),
                                (chroma, spectral.chroma_spec(n_chroma=24), tuning.tuning_spec(), "n_chroma"),
                                (chroma, None, TuningSpec(150.0, 4000.0, 0.1, 2.0, 12, 0), "resolution")):
        with pytest.raises(VsynError) as ei:
            g.pcm_chain_chroma_est_host(None, False, None, None, spec, ch, None, None, est, rates)
        assert word in str(ei.value), str(ei.value)


@pytest.mark.parametrize("output", ["magnitude", "chroma"])
def test_cqt_estimate_equals_explicit_through_synth(mods, submitted, output):
    _, tuning = mods
    from parseoggvorbis_amd import cqt
    from parseoggvorbis_amd.binding import VsynError
    g, S = submitted
    rates = RATES[:S]
    kw = dict(hop_length=256, fmin=110.0, n_bins=24, bins_per_octave=12) if output == "magnitude" else \
        dict(hop_length=256, fmin=110.0, n_bins=36, bins_per_octave=18, output="chroma", n_chroma=6)
    est = tuning.tuning_spec(threshold=0.05, bins_per_octave=kw["bins_per_octave"])
    got = g.pcm_cqt_est_host(cqt.cqt_spec(tuning=-0.3, **kw), est, rates)
    assert got["rc"] == 0 and not got["refused"].any()
    t = got["tuning"]
    assert np.array_equal(t, g.pcm_tuning_host(tuning.framing_spec(2048, 512, power=1), est, rates)["tuning"])
    assert len(set(t.tolist())) > 1, t
    rows = split_rows(got)
    for i in range(S):
        ref = g.pcm_cqt_host(cqt.cqt_spec(tuning=float(t[i]), **kw), rates)
        assert rows[i].shape[0] > 0 and same_bits(rows[i], split_rows(ref)[i]), (output, i, t)
    none = g.pcm_cqt_est_host(cqt.cqt_spec(tuning=float(t[1]), **kw), None, rates)
    assert same_bits(split_rows(none)[1], rows[1]) and not none["tuning"].any()
    with pytest.raises(VsynError) as ei:
        g.pcm_cqt_est_host(cqt.cqt_spec(**kw), tuning.tuning_spec(bins_per_octave=kw["bins_per_octave"] + 1), rates)
    assert "bins_per_octave" in str(ei.value)


def test_estimate_end_to_end_on_ogg_files(mods):
    """get_spectral_batch (chroma, tonnetz), get_cqt_batch and get_chroma_cqt_batch with tuning="estimate" on two files of tests/golden:
    the rows of the same call with the returned tuning, and the tuning get_tuning_batch gives at the matching parameters."""
    spectral, tuning = mods
    from parseoggvorbis_amd import cqt
    from tests.test_gpu_spectral import _ogg
    datas = [_ogg(n) for n in E2E_FILES[:2]]
    for kind in ("chroma", "tonnetz"):
        kw = dict(kind=kind, n_fft=1024, hop_length=256, sr=22050)
        ts = []
        got = spectral.get_spectral_batch(datas, tuning="estimate", tunings=ts, tuning_threshold=0.05, **kw)
        want_t = tuning.get_tuning_batch(datas, n_fft=1024, hop_length=256, power=2, threshold=0.05, sr=22050)
        assert ts == [t for t, _ in want_t] and len(set(ts)) == 2, ts
        for i in range(2):
            assert same_bits(got[i], spectral.get_spectral_batch([datas[i]], tuning=ts[i], **kw)[0]), (kind, i)
        number = []
        spectral.get_spectral_batch(datas, tuning=0.0, tunings=number, **kw)
        assert number == [None, None]
    want_t = [t for t, _ in tuning.get_tuning_batch(datas, n_fft=2048, hop_length=512, power=1, sr=22050)]
    got = cqt.get_cqt_batch(datas, tuning="estimate", n_bins=36, sr=22050)
    assert [e[2] for e in got] == want_t and [e[1] for e in got] == [22050, 22050]
    for i in range(2):
        assert same_bits(got[i][0], cqt.get_cqt_batch([datas[i]], tuning=want_t[i], n_bins=36, sr=22050)[0][0]), i
    want_t = [t for t, _ in tuning.get_tuning_batch(datas, n_fft=2048, hop_length=512, power=1, bins_per_octave=24, sr=22050)]
    kw = dict(n_octaves=3, bins_per_octave=24, fmin=110.0, sr=22050)
    got = cqt.get_chroma_cqt_batch(datas, tuning="estimate", **kw)
    assert [e[2] for e in got] == want_t
    for i in range(2):
        assert same_bits(got[i][0], cqt.get_chroma_cqt_batch([datas[i]], tuning=want_t[i], **kw)[0][0]), i
