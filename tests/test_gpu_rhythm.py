"""The rhythm stages on the device (include/vorbis_synth_hip.h, "rhythm") against the float64 model of tests/rhythm_model.py, through
the device forms on synthetic rows and envelopes.

Gates (tests/rhythm_model.py derives them): an envelope value within one float32 rounding of the model plus 12 e |v| and a flushed
denormal; onset lists equal to the model's, given the same float32 envelope (tests/test_rhythm_cpu.py asserts that every input here
decides its comparisons beyond the band two float64 evaluations can differ in); every tempogram value inside its row's bound; the
mean equal, within (F' + 1) e, to the documented blocked sum of the rows the device itself wrote; the tempo equal to the model's. Each
test prints its worst |d| / bound under pytest -s."""
import itertools

import numpy as np
import pytest

from tests import rhythm_cases as rc
from tests import rhythm_model as rm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def synth():
    import torch
    assert torch.cuda.is_available()
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    yield g
    g.close()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _onset_spec(lag=1, max_size=1, n_fft=2048, hop=512, center=True):
    from parseoggvorbis_amd import binding
    return binding.OnsetSpec(lag, max_size, n_fft, hop, 1 if center else 0)


def _run_onset(g, spec, segs, dim=None):
    """vsyn_onset_strength_device over the segments' rows back to back: the envelopes, one per segment. Three NaN behind the
    envelope must stay NaN, and the rows are read only."""
    import torch
    D = segs[0].shape[1]
    x = np.concatenate(segs) if segs else np.zeros((0, D), np.float32)
    n = len(x)
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_env = torch.full((n + 3,), float("nan"), dtype=torch.float32, device="cuda")
    try:
        g.onset_strength_device(spec, D if dim is None else dim, [len(s) for s in segs], d_in.data_ptr(), d_env.data_ptr(), _stream())
    finally:
        torch.cuda.synchronize()
    env = d_env.cpu().numpy()
    assert np.isnan(env[n:]).all()
    assert np.array_equal(d_in.cpu().numpy(), x, equal_nan=True)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
    return [env[offs[i]:offs[i + 1]] for i in range(len(segs))]


ONSET_P = {0: dict(center=False), 2: dict(n_fft=2048, hop=512), 7: dict(n_fft=1024, hop=73)}


@pytest.mark.parametrize("D", [1, 2, 40, 128, 255, 256])
def test_envelope_against_the_model(synth, D):
    """Every lag x max_size x p: a batch of segments of F in {0, 1, lag, lag + 1, lag + p, lag + p + 1}, one tile of 16 frames
    +- 1 and a longer one. Measured on the MI355X: see DESIGN.md 6p."""
    worst = 0.0
    for lag, m, p in itertools.product((1, 2, 5, 64), (1, 2, 3, 8, 64), (0, 2, 7)):
        kw = dict(lag=lag, max_size=m, **ONSET_P[p])
        assert rm.onset_p(kw.get("n_fft", 2048), kw.get("hop", 512), kw.get("center", True)) == p
        lens = [0, 1, lag, lag + 1, lag + p, lag + p + 1, 15, 16, 17, lag + p + 37]
        segs = [rm.rows(F, D, 1000 * lag + 10 * m + p + 7 * i, kind="db" if i % 2 else "power") for i, F in enumerate(lens)]
        got = _run_onset(synth, _onset_spec(**kw), segs)
        for e, S in zip(got, segs):
            worst = max(worst, rm.onset_gate(e, S, **kw))
        assert np.any(got[-1] > 0)
    print("envelope, D %d: worst |d| / tolerance %.3f" % (D, worst))


def test_envelope_of_non_finite_rows(synth):
    S = rm.rows(40, 40, 5)
    S[7, 3], S[12, 39], S[20, 0], S[30, 17], S[31, 17] = np.nan, np.inf, -np.inf, np.inf, np.inf
    for kw in (dict(lag=1, center=False), dict(lag=2, max_size=5), dict(lag=1, max_size=64, center=False)):
        got = _run_onset(synth, _onset_spec(**kw), [S, rm.rows(9, 40, 6)])
        rm.onset_gate(got[0], S, **kw)
        rm.onset_gate(got[1], rm.rows(9, 40, 6), **kw)
        assert np.isnan(got[0]).any() and np.isinf(got[0]).any() and not np.isnan(got[1]).any()


@pytest.mark.parametrize("D", [40, 255])
def test_envelope_same_rows_same_bits(synth, D):
    kw = dict(lag=2, max_size=3)
    for F in (5, 33, 130):
        X = rm.rows(F, D, 11 + F)
        alone = _run_onset(synth, _onset_spec(**kw), [X])[0]
        lens = [F, 130, 1, F, 0, 63, 70, F, 64]
        for fill in (None, 1e30):
            segs = [X if j in (0, 3, 7) else rm.rows(n, D, 31 + j) if fill is None else np.full((n, D), fill, np.float32) for j, n in enumerate(lens)]
            got = _run_onset(synth, _onset_spec(**kw), segs)
            for j in (0, 3, 7):
                assert np.array_equal(got[j], alone), (D, F, j, fill)


def test_envelope_refusals_leave_the_output_alone(synth):
    from parseoggvorbis_amd import binding
    S = rm.rows(20, 8, 1)
    for kw, dim in ((dict(lag=0), None), (dict(lag=65), None), (dict(max_size=0), None), (dict(max_size=65), None), (dict(hop=0), None),
                    (dict(n_fft=0), None), ({}, 0), ({}, 257)):
        with pytest.raises(binding.VsynError) as ei:
            _run_onset(synth, _onset_spec(**kw), [S], dim=dim)
        assert ei.value.code == binding.VSYN_ERR_INVALID, (kw, dim)
    bad = _onset_spec()
    bad.options = 2
    with pytest.raises(binding.VsynError):
        _run_onset(synth, bad, [S])


# ---- onset frames ---------------------------------------------------------------------------------------------------------------
def _peaks_spec(times, delta, hop, normalize):
    from parseoggvorbis_amd import binding
    return binding.OnsetPeaks(times["pre_max"], times["post_max"], times["pre_avg"], times["post_avg"], times["wait"], delta, hop, 1 if normalize else 0)


def _run_peaks(g, spec, envs, rates):
    """vsyn_onset_peaks_device: (list of int64 frame arrays, refused [S]). Words behind a segment's count keep their fill."""
    import torch
    x = np.concatenate(envs) if envs else np.zeros(0, np.float32)
    n, S = len(x), len(envs)
    d_env = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    fill = 0xDEADBEEF - (1 << 32)
    d_on = torch.full((n + 3,), fill, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((S + 1,), fill, dtype=torch.int32, device="cuda")
    d_ref = torch.full((S + 1,), fill, dtype=torch.int32, device="cuda")
    try:
        g.onset_peaks_device(spec, [len(e) for e in envs], rates, d_env.data_ptr(), d_on.data_ptr(), d_cnt.data_ptr(), d_ref.data_ptr(), _stream())
    finally:
        torch.cuda.synchronize()
    on, cnt, ref = d_on.cpu().numpy(), d_cnt.cpu().numpy(), d_ref.cpu().numpy()
    assert cnt[S] == fill and ref[S] == fill and np.all(on[n:] == fill)
    assert np.array_equal(d_env.cpu().numpy(), x, equal_nan=True)
    offs = np.concatenate([[0], np.cumsum([len(e) for e in envs])])
    out = []
    for i in range(S):
        assert 0 <= cnt[i] <= len(envs[i])
        assert np.all(on[offs[i] + cnt[i]:offs[i + 1]] == fill)
        out.append(on[offs[i]:offs[i] + cnt[i]].astype(np.int64))
    return out, ref[:S]


CASES = rc.peak_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_peaks_equal_the_models(synth, case):
    _, x, rate, hop, times, delta, normalize = case
    want, refused = rm.peak_pick(x, rm.peak_windows(rate, hop, **times), delta, normalize)
    got, ref = _run_peaks(synth, _peaks_spec(times, delta, hop, normalize), [x], [rate])
    assert not refused and ref[0] == 0
    assert np.array_equal(got[0], want), (len(got[0]), len(want))


def test_peaks_in_a_batch_and_a_refused_segment(synth):
    """Segments of different lengths and rates in one call, an empty one and a skipped one (rate 0) among them; the one that holds a
    NaN, and the one that holds an Inf, are refused alone."""
    envs = [rm.click_train(), rm.envelope(4097, 3), np.zeros(0, np.float32), rm.click_train(period=37, first=11), rm.envelope(65, 4), rm.envelope(64, 5),
            rm.envelope(130, 6), rm.envelope(63, 8)]
    envs[4][64] = np.nan
    envs[6][0] = np.inf
    rates = [22050, 44100, 22050, 44100, 22050, 16000, 48000, 0]
    spec = _peaks_spec(rm.PEAK_TIMES, 0.07, 512, True)
    got, ref = _run_peaks(synth, spec, envs, rates)
    assert list(ref) == [0, 0, 0, 0, 1, 0, 1, 0]
    for e, r, o in zip(envs, rates, got):
        want = rm.peak_pick(e, rm.peak_windows(r, 512), 0.07, True)[0] if r else np.zeros(0, np.int64)
        assert np.array_equal(o, want)
    assert np.array_equal(got[0], np.arange(5, 600, 20)) and len(got[1]) > 100 and len(got[7]) == 0


def test_peaks_refusals(synth):
    from parseoggvorbis_amd import binding
    x = rm.envelope(30, 1)
    for bad in (dict(pre_max=-0.1), dict(wait=np.inf), dict(pre_avg=1e6)):
        with pytest.raises(binding.VsynError) as ei:
            _run_peaks(synth, _peaks_spec(dict(rm.PEAK_TIMES, **bad), 0.07, 512, True), [x], [22050])
        assert ei.value.code == binding.VSYN_ERR_INVALID
    with pytest.raises(binding.VsynError):
        _run_peaks(synth, _peaks_spec(rm.PEAK_TIMES, np.nan, 512, True), [x], [22050])


# ---- tempogram, mean, tempo -----------------------------------------------------------------------------------------------------
def _tg_spec(W=384, center=True, norm=True, hop=512, ac_size=8.0):
    from parseoggvorbis_amd import binding
    return binding.TempogramSpec(W, hop, (1 if center else 0) | (2 if norm else 0), 0, ac_size)


def _run_tg(g, spec, envs, Ws, rates=None, rows=True, mean=True):
    """vsyn_tempogram_device: (list of (F', W) float32 or None, list of g float64 or None). Three NaN behind each output stay."""
    import torch
    center = bool(spec.options & 1)
    x = np.concatenate(envs) if envs else np.zeros(0, np.float32)
    fps = [rm.tg_rows(len(e), W, center) for e, W in zip(envs, Ws)]
    nr, nm = sum(f * W for f, W in zip(fps, Ws)), sum(Ws)
    d_env = torch.from_numpy(np.ascontiguousarray(x)).cuda() if len(x) else torch.zeros(1, device="cuda")
    d_rows = torch.full((nr + 3,), float("nan"), dtype=torch.float32, device="cuda") if rows else None
    d_mean = torch.full((nm + 3,), float("nan"), dtype=torch.float64, device="cuda") if mean else None
    try:
        g.tempogram_device(spec, [len(e) for e in envs], rates, d_env.data_ptr(), d_rows.data_ptr() if rows else None,
                           d_mean.data_ptr() if mean else None, _stream())
    finally:
        torch.cuda.synchronize()
    out_r = out_m = None
    if rows:
        r = d_rows.cpu().numpy()
        assert np.isnan(r[nr:]).all()
        o = np.concatenate([[0], np.cumsum([f * W for f, W in zip(fps, Ws)])])
        out_r = [r[o[i]:o[i + 1]].reshape(fps[i], Ws[i]) for i in range(len(envs))]
    if mean:
        m = d_mean.cpu().numpy()
        assert np.isnan(m[nm:]).all()
        o = np.concatenate([[0], np.cumsum(Ws)])
        out_m = [m[o[i]:o[i + 1]] for i in range(len(envs))]
    return out_r, out_m


def _some_rows(Fp, ft, seed):
    """All rows of a short segment; of a long one its ends, both sides of the tile boundaries in its middle, and a dozen others."""
    if Fp <= 40:
        return None
    mid = (Fp // 2) // ft * ft
    pick = set(range(6)) | set(range(Fp - 6, Fp)) | {mid - 1, mid, mid + ft - 1, mid + ft}
    pick |= set(int(v) for v in np.random.default_rng(seed).integers(0, Fp, 12))
    return sorted(f for f in pick if 0 <= f < Fp)


def _gate_mean(g, rows):
    """The device mean against the documented blocked sum of the rows the device wrote: (F' + 1) e mean|row|."""
    want = rm.tg_mean(rows)
    if len(rows) == 0:
        assert np.isnan(g).all()
        return 0.0
    tol = (len(rows) + 1) * rm.E64 * np.abs(rows.astype(np.float64)).mean(axis=0) + 2.0 ** -1074
    d = np.abs(g - want)
    assert np.all(d <= tol), float((d / tol).max())
    return float((d / tol).max())


@pytest.mark.parametrize("norm", [True, False], ids=["inf", "none"])
@pytest.mark.parametrize("W", [2, 3, 16, 384, 689, 2048])
def test_tempogram_against_the_model(synth, W, norm):
    """Centred: F in {1, W/2 - 1, W/2, W/2 + 1, W, one tile - 1, one tile, one tile + 1} and an empty segment in one call, one of them
    negative-valued. At W >= 689 the model (W^2 a frame) gates the rows _some_rows() names; the mean is gated on all rows."""
    ft = rm.tg_tile(W)
    lens = sorted(set(F for F in (1, W // 2 - 1, W // 2, W // 2 + 1, W, ft - 1, ft, ft + 1) if F >= 1)) + [0]
    envs = [rm.envelope(F, 100 * W + F, negative=(i == 2)) for i, F in enumerate(lens)]
    rows, means = _run_tg(synth, _tg_spec(W, True, norm), envs, [W] * len(envs))
    worst = worst_g = 0.0
    for i, e in enumerate(envs):
        worst = max(worst, rm.tg_gate(rows[i], e, W, True, norm, only=_some_rows(len(e), ft, W + i)))
        worst_g = max(worst_g, _gate_mean(means[i], rows[i]))
        if norm and len(e):
            assert np.all(np.abs(rows[i]).max(axis=1) == 1.0)
    print("tempogram W %d norm %s: worst |d| / bound %.3f, mean %.3f" % (W, norm, worst, worst_g))


@pytest.mark.parametrize("W", [16, 384])
def test_tempogram_uncentred_and_outputs_alone(synth, W):
    """tg_center off: F < W gives no rows, F = W one; rows alone and the mean alone are the rows and the mean of the call that asks for both."""
    lens = [W - 1, W, W + 1, W + 2 * rm.tg_tile(W) + 1, 0, 5]
    envs = [rm.envelope(F, 7 * W + F) for F in lens]
    spec = _tg_spec(W, False, True)
    rows, means = _run_tg(synth, spec, envs, [W] * len(envs))
    assert [len(r) for r in rows] == [0, 1, 2, 2 * rm.tg_tile(W) + 2, 0, 0]
    for i, e in enumerate(envs):
        rm.tg_gate(rows[i], e, W, False, True)
        _gate_mean(means[i], rows[i])
    only_r, none = _run_tg(synth, spec, envs, [W] * len(envs), mean=False)
    assert none is None and all(np.array_equal(a, b) for a, b in zip(only_r, rows))
    none, only_m = _run_tg(synth, spec, envs, [W] * len(envs), rows=False)
    assert none is None and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(only_m, means))


def test_tempogram_zero_and_non_finite_envelopes(synth):
    z = np.zeros(40, np.float32)
    e = rm.envelope(40, 2)
    e[20] = np.nan
    i = rm.envelope(40, 3)
    i[9] = np.inf
    for norm in (True, False):
        rows, means = _run_tg(synth, _tg_spec(8, True, norm), [z, e, i], [8, 8, 8])
        assert not rows[0].any() and not means[0].any()  # zero rows are not divided
        rm.tg_gate(rows[1], e, 8, True, norm)
        want, _ = rm.tempogram(i, 8, True, norm)
        assert np.array_equal(np.isnan(rows[2]), np.isnan(want)) and np.array_equal(np.isinf(rows[2]), np.isinf(want))
        if norm:
            assert np.array_equal(np.isnan(rows[1]).all(axis=1), [17 <= f <= 24 for f in range(40)])
            assert np.isnan(means[1]).all()


def test_tempogram_same_envelope_same_bits(synth):
    """Rows and mean of a segment alone, and as segment 0, 3 and 6 of a batch of other lengths, other values and another W."""
    W = 384
    for F in (30, 600):
        e = rm.click_train(F=F) if F == 600 else rm.envelope(F, 9)
        spec = _tg_spec(0, True, True, hop=512, ac_size=384 * 512 / 22050 + 1e-9)
        assert spec.win_length == 0
        alone_r, alone_m = _run_tg(synth, spec, [e], [W], rates=[22050])
        envs = [e, np.full(70, 1e30, np.float32), rm.envelope(1, 1), e, np.zeros(0, np.float32), np.full(500, 1e30, np.float32), e]
        rates = [22050, 22050, 44100, 22050, 8000, 11025, 22050]
        Ws = [int(np.floor(spec.ac_size * r / 512)) for r in rates]
        assert Ws[0] == W and len(set(Ws)) == 4
        rows, means = _run_tg(synth, spec, envs, Ws, rates=rates)
        for j in (0, 3, 6):
            assert np.array_equal(rows[j], alone_r[0]) and np.array_equal(means[j], alone_m[0])


def test_tempogram_skips_a_segment_of_rate_zero(synth):
    """win_length 0: a rate of 0 skips the segment, which then has neither rows nor mean values; a call of skipped segments alone
    launches nothing."""
    e = rm.envelope(50, 4)
    spec = _tg_spec(0, True, True, hop=512, ac_size=16 * 512 / 22050 + 1e-9)
    rows, means = _run_tg(synth, spec, [e, e, e], [0, 16, 0], rates=[0, 22050, 0])
    assert rows[0].size == rows[2].size == means[0].size == means[2].size == 0
    rm.tg_gate(rows[1], e, 16)
    rows, means = _run_tg(synth, spec, [e, e], [0, 0], rates=[0, 0])
    assert rows[0].size == means[1].size == 0


TEMPO = rc.tempo_cases()


@pytest.mark.parametrize("case", TEMPO, ids=[c[0] for c in TEMPO])
def test_tempo_of_the_click_trains(synth, case):
    """The mean alone off the device, then the library's host arithmetic: the model's lag and bpm."""
    from parseoggvorbis_amd import binding
    _, e, rate, hop, W, kw = case
    _, means = _run_tg(synth, _tg_spec(W, True, True, hop=hop), [e], [W], rows=False)
    rows, bound = rm.tempogram(e, W)
    d = np.abs(means[0] - rm.tg_mean(rows))
    assert np.all(d <= rm.tg_mean_bound(rows, bound))
    spec = binding.TempoSpec(kw.get("start_bpm", 120.0), kw.get("std_bpm", 1.0), kw.get("max_tempo", 320.0) or 0.0)
    bpm, lag, margin, band = rm.tempo(rm.tg_mean(rows), rate, hop, **kw)
    assert binding.tempo_from_mean(spec, means[0], rate, hop) == (bpm, lag)
    print("tempo %s: %.4f bpm at lag %d; mean worst |d| / bound %.3f" % (case[0], bpm, lag, float((d / rm.tg_mean_bound(rows, bound)).max())))


def test_tempogram_refusals(synth):
    from parseoggvorbis_amd import binding
    e = rm.envelope(30, 1)
    for spec, rates in ((_tg_spec(1), None), (_tg_spec(2049), None), (_tg_spec(0, ac_size=8.0), [192000]), (_tg_spec(0, ac_size=np.nan), [22050]),
                        (_tg_spec(0, ac_size=8.0), None), (_tg_spec(16, hop=0), None)):
        with pytest.raises(binding.VsynError) as ei:
            _run_tg(synth, spec, [e], [16], rates=rates)
        assert ei.value.code == binding.VSYN_ERR_INVALID
    with pytest.raises(binding.VsynError):
        _run_tg(synth, _tg_spec(16), [e], [16], rows=False, mean=False)


# ---- the host chain ---------------------------------------------------------------------------------------------------------------
def test_host_chain():
    """rhythm = NULL is vsyn_pcm_chain_hpss_host; with a spec every output is the device forms' on that entry's rows, bit for bit,
    ungated, trimmed and split; delta / normalize and a kind wider than 256 columns are refused by name."""
    from parseoggvorbis_amd import binding, rhythm, spectral
    from parseoggvorbis_amd.binding import PcmCond, PcmTrim, SpectralPost, Synth, VsynError
    from tests.workloads import fixture_like_spec, synth_batch
    setup = fixture_like_spec(2)
    b = synth_batch(setup, streams=3, packets_per_stream=12, pattern="mixed", seed=11)
    S = len(b["segments"])
    rates = ([44100, 22050, 44100] + [44100] * S)[:S]
    g = Synth(setup, device=0, max_streams=4)
    try:
        assert g.submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"], flags=4)["rc"] == 0
        s = spectral.spectral_spec(kind="mel_power", power=1, n_fft=400, hop_length=160, n_mels=40)
        hp = spectral.hpss_spec("percussive", (9, 5))
        c = type("C", (), dict(spec=s))

        def spec_of(output, **kw):
            return rhythm._rhythm_spec(output, c, 2, 3, **kw)
        for gate, is_split, cond in ((None, 0, None), (PcmTrim(256, 64, 40.0), 0, PcmCond(1, 0, 0.0)), (PcmTrim(256, 64, 40.0), 1, PcmCond(1, 0, 0.0))):
            plain = g.pcm_chain_hpss_host(gate, is_split, None, cond, s, None, hp, None, None, rates)
            off = g.pcm_chain_rhythm_host(gate, is_split, None, cond, s, None, hp, None, None, None, rates)
            assert off["rc"] == 0 and plain["rows"].shape[0] > 0
            for k in ("rows", "seg_rows", "bounds", "frames", "counts", "peaks", "refs"):
                assert np.array_equal(off[k], plain[k]), k
            nrows = [int(n) for n in plain["seg_rows"]]
            offs = np.concatenate([[0], np.cumsum(nrows)])
            segs = [plain["rows"][offs[i]:offs[i + 1]] for i in range(S)]
            env = _run_onset(g, _onset_spec(2, 3, 400, 160, True), segs)
            r = g.pcm_chain_rhythm_host(gate, is_split, None, cond, s, None, hp, None, None, spec_of("envelope"), rates)
            assert r["rc"] == 0 and np.array_equal(r["seg_rows"], plain["seg_rows"]) and np.array_equal(r["rows"][:, 0], np.concatenate(env))
            assert np.array_equal(r["bounds"], plain["bounds"]) and np.array_equal(r["frames"], plain["frames"])
            want, refused = _run_peaks(g, _peaks_spec(rm.PEAK_TIMES, 0.07, 160, True), env, rates)
            r = g.pcm_chain_rhythm_host(gate, is_split, None, cond, s, None, hp, None, None, spec_of("onsets", peaks={}), rates)
            assert [int(n) for n in r["seg_rows"]] == [len(w) for w in want] and not refused.any() and not r["refused"].any()
            assert np.array_equal(r["rows"].view(np.uint32)[:, 0].astype(np.int64), np.concatenate(want))
            tg, _ = _run_tg(g, _tg_spec(32, True, True, hop=160), env, [32] * S, mean=False)
            r = g.pcm_chain_rhythm_host(gate, is_split, None, cond, s, None, hp, None, None, spec_of("tempogram", tempogram=dict(win_length=32)), rates)
            assert np.array_equal(r["seg_rows"], plain["seg_rows"]) and np.array_equal(r["rows"], np.concatenate(tg))
            ts = _tg_spec(0, True, True, hop=160, ac_size=0.25)
            Ws = [int(np.floor(0.25 * x / 160)) for x in rates]
            _, means = _run_tg(g, ts, env, Ws, rates=rates, rows=False)
            r = g.pcm_chain_rhythm_host(gate, is_split, None, cond, s, None, hp, None, None,
                                        spec_of("tempo_mean", tempogram=dict(win_length=None, ac_size=0.25)), rates)
            assert [int(n) for n in r["seg_rows"]] == [w + 1 for w in Ws]
            want = np.concatenate([np.concatenate([m, [float(x)]]) for m, x in zip(means, rates)])
            assert np.array_equal(np.ascontiguousarray(r["rows"]).view(np.float64)[:, 0], want, equal_nan=True)
        post = SpectralPost(2, 3, 2, 0, 1e-5, None, None)
        with pytest.raises(VsynError, match="delta / normalize"):
            g.pcm_chain_rhythm_host(None, 0, None, None, s, None, None, None, post, spec_of("envelope"), rates)
        wide = spectral.spectral_spec(kind="lin_power", n_fft=1024, hop_length=160)
        c.spec = wide
        with pytest.raises(VsynError, match="256"):
            g.pcm_chain_rhythm_host(None, 0, None, None, wide, None, None, None, None, spec_of("envelope"), rates)
        mismatch = spec_of("envelope")
        with pytest.raises(VsynError, match="spectral spec"):
            g.pcm_chain_rhythm_host(None, 0, None, None, s, None, None, None, None, mismatch, rates)
    finally:
        g.close()


# ---- end to end from Ogg bytes --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from parseoggvorbis_amd import rhythm, spectral
    return rhythm, spectral


@pytest.fixture(scope="module")
def blobs():
    """The two real fixtures, and the mono one re-headed to 16 kHz so that the rates differ within a call."""
    from tests.test_gpu_spectral import _ogg, _rehead
    real = [_ogg("test.stereo44khz"), _ogg("test.mono44khz")]
    return real + [_rehead(real[1], 16000)]


SMALL = dict(n_fft=400, hop_length=160, n_mels=40)
E2E = [dict(), dict(sr=16000), dict(trim_db=30.0), dict(SMALL, kind="mel_power", hpss="percussive"),
       dict(SMALL, kind="mel_power", hpss="percussive", sr=16000, trim_db=30.0)]


@pytest.mark.parametrize("kw", E2E, ids=lambda k: "-".join("%s=%s" % (a, k[a]) for a in ("kind", "sr", "trim_db", "hpss") if a in k) or "defaults")
def test_end_to_end_from_ogg_bytes(mods, blobs, kw):
    """The envelope against the model on the rows get_spectral_batch returns for the same arguments; onsets, tempogram, mean and tempo
    against the model on that envelope. The comparisons of the peak picker and of the tempo are checked to be decided first."""
    from tests.test_gpu_spectral import _rate
    rhythm, spectral = mods
    n_fft, hop = kw.get("n_fft", 2048), kw.get("hop_length", 512)
    rates = [kw.get("sr") or _rate(b) for b in blobs]
    rows = spectral.get_spectral_batch(blobs, **dict(dict(kind="mel_db"), **kw))
    okw = dict(lag=2, max_size=3)
    env = rhythm.get_onset_strength_batch(blobs, **okw, **kw)
    worst = 0.0
    for e, S in zip(env, rows):
        assert len(e) == len(S) > 20
        worst = max(worst, rm.onset_gate(e, S, n_fft=n_fft, hop=hop, center=True, **okw))
    envs = []
    onsets = rhythm.get_onsets_batch(blobs, envelope=envs, **okw, **kw)
    tg = rhythm.get_tempogram_batch(blobs, win_length=64, **okw, **kw)
    means = []
    tempo = rhythm.get_tempo_batch(blobs, ac_size=2.0, tempogram_mean=means, **okw, **kw)
    for i, e in enumerate(env):
        assert np.array_equal(envs[i], e)
        w = rm.peak_windows(rates[i], hop)
        assert rm.band_b(e, w) > 1.0
        assert onsets[i].dtype == np.int64 and np.array_equal(onsets[i], rm.peak_pick(e, w)[0])
        rm.tg_gate(tg[i], e, 64)
        W = int(np.floor(2.0 * rates[i] / hop))
        want_rows, bound = rm.tempogram(e, W)
        assert means[i].shape == (W,) and np.all(np.abs(means[i] - rm.tg_mean(want_rows)) <= rm.tg_mean_bound(want_rows, bound))
        bpm, lag, margin, band = rm.tempo(means[i], rates[i], hop)
        assert margin > band and tempo[i] == (bpm, rates[i])
    print("end to end %r: envelope worst |d| / tolerance %.3f, onsets %r, tempo %r" % (kw, worst, [len(o) for o in onsets], tempo))


def test_a_damaged_file_fails_alone_and_the_spectral_call_is_unchanged(mods, blobs):
    rhythm, spectral = mods
    names = [0, 1, 2] * 2
    data = [blobs[i] for i in names]
    bad = bytearray(data[4])
    bad[len(bad) // 2] ^= 0x55  # a page CRC
    data[4] = bytes(bad)
    single = [rhythm.get_onsets_from_raw_bytes(b) for b in blobs]
    singles_t = [rhythm.get_tempo_from_raw_bytes(b) for b in blobs]
    res = rhythm.get_onsets_batch(data, errors="return", files_per_submit=4)
    tempos = rhythm.get_tempo_batch(data, errors="return", files_per_submit=4)
    for i, n in enumerate(names):
        if i == 4:
            assert isinstance(res[i], rhythm.RhythmError) and "file 4" in str(res[i]) and isinstance(tempos[i], rhythm.RhythmError)
            continue
        assert np.array_equal(res[i], single[n]) and tempos[i] == singles_t[n]
    with pytest.raises(rhythm.RhythmError):
        rhythm.get_onset_strength_batch(data)
    # a window length outside [2, 2048] fails that file alone: 60 s at 44100 / 512 are 5167 frames, at 16000 / 512 1875
    t = rhythm.get_tempo_batch(blobs, ac_size=60.0, errors="return")
    assert isinstance(t[0], rhythm.RhythmError) and isinstance(t[1], rhythm.RhythmError) and "2048" in str(t[0]) and isinstance(t[2], tuple)
    # the rows of an existing test's arguments, bit for bit what they are through the entry get_spectral_batch takes for them
    from parseoggvorbis_amd import binding
    MEL = dict(kind="mel_power", power=1, n_fft=400, hop_length=160, n_mels=40)
    a = spectral.get_spectral_batch(blobs, **MEL)
    b = spectral.get_spectral_batch(blobs, hpss="percussive", hpss_output="median", hpss_kernel_size=(1, 1), **MEL)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)  # the median of one element is the element: the HPSS entry's rows, which the rhythm entry shares
    assert "vsyn_pcm_chain_rhythm_host" in binding.declared_symbols()
