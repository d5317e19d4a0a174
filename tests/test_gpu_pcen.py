"""PCEN on the device (include/vorbis_synth_hip.h, "PCEN") against the float64 model of tests/pcen_model.py.

The gate, per element and with nothing left out: |d| <= 2 u |Y| + 2^-126, u = 2^-24 (tests/pcen_model.py gate()): one rounding to
float32, the float64 recurrence and library functions (non-negative terms, a few ulp of float64 each, conditioned by
gain |log eps| < 30: below 2^-40 relative), and a flushed denormal. The NumPy restatement of the device's blocked order
(tests/test_pcen_cpu.py) sits at 0.995 u |Y|, the device at 1.000 (the figures are in the tests' docstrings; each test prints its
own under pytest -s).

(1) the stage alone over D x parameter sets x scales, nine segments a call, b given and derived from two rates; (2) in place = out of
place; (3) same rows, same bits, wherever the segment lies; (4) a segment of 313 blocks; (5) refusals with the output untouched;
(6) the host forms: pcen = NULL is the entry without it, with a spec it is the stage alone on that entry's rows, then the post
stage's, and the PCM and the next submit are left alone; (7) get_spectral_batch end to end."""
import numpy as np
import pytest

from tests import pcen_model as pm
from tests.test_gpu_spectral import _ogg, _rate, _rehead

pytestmark = pytest.mark.gpu

HOP = 160
RATES = (16000, 44100)


@pytest.fixture(scope="module")
def spec_mod():
    import torch
    assert torch.cuda.is_available()
    from parseoggvorbis_amd import spectral
    return spectral


@pytest.fixture(scope="module")
def synth():
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    yield g
    g.close()


def _spec(**kw):
    from parseoggvorbis_amd import spectral
    kw = dict(pm.DEFAULTS, **kw)
    return spectral.pcen_spec(kw["gain"], kw["bias"], kw["power"], kw["time_constant"], kw["eps"], kw["b"], kw["scale"])


def _run_stage(g, pc, x, seg_rows, rates, hop=HOP, in_place=False, dim=None):
    """vsyn_spectral_pcen_device over rows x (total, D) float32 split as seg_rows: (total, D) float32. Three rows of NaN behind the
    rows must stay NaN."""
    import torch
    n, D = x.shape
    pad = np.full((3, D), np.nan, np.float32)
    d_in = torch.from_numpy(np.concatenate([np.ascontiguousarray(x), pad])).cuda()
    d_out = d_in if in_place else torch.full((n + 3, D), float("nan"), dtype=torch.float32, device="cuda")
    try:
        g.spectral_pcen_device(pc, D if dim is None else dim, seg_rows, rates, hop, d_in.data_ptr(), d_out.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    finally:
        torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.isnan(out[n:]).all()  # nothing written past the rows
    return out[:n]


def _batch(D, seed, scale, seg_rows=pm.SEG_ROWS):
    return [pm.rows(F, D, seed + 17 * i, scale) for i, F in enumerate(seg_rows)]


def _gate_segments(got, segs, rates, kw):
    worst, o = 0.0, 0
    for i, X in enumerate(segs):
        worst = max(worst, pm.gate(got[o:o + len(X)], X, sr=rates[i], hop_length=HOP, **kw))
        o += len(X)
    assert o == len(got)
    return worst


@pytest.mark.parametrize("D", [1, 4, 40, 128, 256, 257, 513])
def test_stage_alone_against_the_model(synth, D):
    """(1) Measured on the MI355X, worst |d| / (u |Y|) over the seven parameter sets and both scales: D = 1 0.988, 4 0.995, 40 0.999,
    128 0.999, 256 1.000, 257 1.000, 513 0.999: the one rounding to float32; the float64 terms do not show."""
    S = len(pm.SEG_ROWS)
    rates = [RATES[i % 2] for i in range(S)]
    worst = 0.0
    for i, p in enumerate(pm.PARAMS):
        for scale in (1.0, 2.0 ** 31):
            kw = dict(pm.DEFAULTS, scale=scale, **p)
            segs = _batch(D, 100 * i + D, scale)
            # a given b needs no rates: NULL on every other parameter set
            got = _run_stage(synth, _spec(**kw), np.concatenate(segs), pm.SEG_ROWS, None if kw["b"] is not None and i % 2 == 0 else rates)
            assert not np.isnan(got).any()
            worst = max(worst, _gate_segments(got, segs, rates, kw))
    print("stage alone, D %d: worst |d| / (u |Y|) %.3f (gate 2)" % (D, worst))
    assert worst > 0.5  # the rows are not trivial


def test_derived_coefficients_differ_between_the_rates(synth):
    X = pm.rows(200, 8, 5)
    a = _run_stage(synth, _spec(), X, [200], [RATES[0]])
    b = _run_stage(synth, _spec(), X, [200], [RATES[1]])
    assert not np.array_equal(a, b)
    both = _run_stage(synth, _spec(), np.concatenate([X, X]), [200, 200], list(RATES))
    assert np.array_equal(both[:200], a) and np.array_equal(both[200:], b)
    # a rate of 0 skips its segment: its rows are not written
    skip = _run_stage(synth, _spec(), np.concatenate([X, X]), [200, 200], [0, RATES[1]])
    assert np.isnan(skip[:200]).all() and np.array_equal(skip[200:], b)


@pytest.mark.parametrize("D", [4, 257])
def test_in_place_equals_out_of_place(synth, D):
    """(2)"""
    for i in (0, 1, 2, 5):
        kw = dict(pm.DEFAULTS, scale=2.0 ** 31, **pm.PARAMS[i])
        x = np.concatenate(_batch(D, 7 + i, kw["scale"]))
        rates = [RATES[j % 2] for j in range(len(pm.SEG_ROWS))]
        out = _run_stage(synth, _spec(**kw), x, pm.SEG_ROWS, rates)
        assert np.array_equal(_run_stage(synth, _spec(**kw), x, pm.SEG_ROWS, rates, in_place=True), out), (D, i)


@pytest.mark.parametrize("D", [40, 513])
def test_same_rows_same_bits_wherever_the_segment_lies(synth, D):
    """(3) a segment alone, and the same rows as segment 0, 3 and 7 of a batch of other lengths."""
    kw = dict(pm.DEFAULTS, b=0.03)
    for F in (65, 1000):
        X = pm.rows(F, D, 11 + F)
        alone = _run_stage(synth, _spec(**kw), X, [F], None)
        lens = [F, 130, 1, F, 0, 63, 700, F, 64]
        segs = [X if j in (0, 3, 7) else pm.rows(n, D, 31 + j) for j, n in enumerate(lens)]
        got = _run_stage(synth, _spec(**kw), np.concatenate(segs), lens, None)
        again = _run_stage(synth, _spec(**kw), np.concatenate(segs), lens, None)
        assert np.array_equal(got, again)
        offs = np.concatenate([[0], np.cumsum(lens)])
        for j in (0, 3, 7):
            assert np.array_equal(got[offs[j]:offs[j] + F], alone), (D, F, j)


def test_long_segment(synth):
    """(4) F = 20 000, D = 2, b = 1e-3: 313 blocks through the carry kernel. Measured: worst |d| / (u |Y|) 0.992."""
    kw = dict(pm.DEFAULTS, b=1e-3)
    X = pm.rows(20000, 2, 3)
    X[:, 0] = pm.rows(20000, 3, 4)[:, 1]  # a live column, and one that falls silent at row 64: the carries alone hold it up
    got = _run_stage(synth, _spec(**kw), X, [20000], None)
    worst = pm.gate(got, X, **kw)
    print("long segment: worst |d| / (u |Y|) %.3f (gate 2)" % worst)
    assert worst > 0.5


def test_stage_refuses_bad_arguments_and_writes_nothing(synth):
    """(5)"""
    from parseoggvorbis_amd.binding import VsynError
    x = pm.rows(20, 8, 1)
    cases = []
    for field, values in (("gain", (-1.0, np.inf, np.nan)), ("bias", (-1.0, np.nan)), ("power", (-1.0, np.inf)), ("eps", (0.0, -1.0, np.nan)),
                          ("time_constant", (0.0, np.inf)), ("scale", (0.0, -2.0, np.inf)), ("b", (-0.5, 1.5, np.nan))):
        for v in values:
            pc = _spec()
            setattr(pc, field, v)
            cases.append((pc, dict(rates=[44100])))
    cases.append((_spec(), dict(rates=None)))          # b = 0 with NULL rates
    cases.append((_spec(), dict(rates=[44100], hop=0)))  # b = 0 with hop_length = 0
    cases.append((_spec(b=0.5), dict(rates=None, dim=0)))
    cases.append((None, dict(rates=[44100])))
    for pc, kw in cases:
        with pytest.raises(VsynError) as ei:
            _run_stage(synth, pc, x, [20], **kw)
        assert ei.value.code == 1, str(ei.value)  # VSYN_ERR_INVALID
    # (_run_stage fills the output with NaN first; a refused call must leave it so)
    import torch
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.full((20, 8), float("nan"), dtype=torch.float32, device="cuda")
    for pc, kw in cases:
        with pytest.raises(VsynError):
            synth.spectral_pcen_device(pc, kw.get("dim", 8), [20], kw["rates"], kw.get("hop", HOP), d_in.data_ptr(), d_out.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.isnan(d_out.cpu().numpy()).all()
    synth.spectral_pcen_device(_spec(b=0.5), 8, [20], None, 0, d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), _run_stage(synth, _spec(b=0.5), x, [20], None))


def _post_stage(g, post, x, seg_rows):
    import torch
    D = x.shape[1]
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.full((x.shape[0], D * (1 + post.order)), float("nan"), dtype=torch.float32, device="cuda")
    g.spectral_post_device(post, D, seg_rows, d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def test_host_forms(spec_mod):
    """(6)"""
    from parseoggvorbis_amd.binding import PcmCond, PcmTrim, SpectralPost, Synth, VsynError, VSYN_PCM_F32
    from tests.workloads import fixture_like_spec, synth_batch
    spec = fixture_like_spec(2)
    b1 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=11)
    b2 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=12)
    S = len(b1["segments"])
    rates = [44100, 22050, 44100][:S] + [44100] * max(0, S - 3)
    post = SpectralPost(2, 3, 2, 0, 1e-5, None, None)  # delta 2 over width 3, mean_var
    pc = _spec(scale=2.0 ** 31)
    outs = []
    for with_pcen in (False, True):
        g = Synth(spec, device=0, max_streams=4)
        r1 = g.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"], flags=4)  # KEEP_PCM
        assert r1["rc"] == 0
        f1, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        if with_pcen:
            for kw in (dict(kind="mel_power", power=1, n_fft=400, hop_length=160, n_mels=40), dict(kind="lin_power", n_fft=256, hop_length=64)):
                s = spec_mod.spectral_spec(**kw)
                for trim, cond in ((None, None), (PcmTrim(256, 64, 40.0), PcmCond(1, 0, 0.0))):
                    plain = g.pcm_trim_spectral_host(trim, cond, s, None, rates)
                    off = g.pcm_trim_spectral_pcen_host(trim, cond, s, None, None, rates)
                    assert off["rc"] == 0 and np.array_equal(off["rows"], plain["rows"]) and np.array_equal(off["seg_rows"], plain["seg_rows"])
                    assert np.array_equal(off["bounds"], plain["bounds"]) and plain["rows"].shape[0] > 0
                    on = g.pcm_trim_spectral_pcen_host(trim, cond, s, pc, None, rates)
                    want = _run_stage(g, pc, plain["rows"], plain["seg_rows"], rates, hop=s.hop_length)
                    assert on["rc"] == 0 and np.array_equal(on["seg_rows"], plain["seg_rows"]) and np.array_equal(on["rows"], want)
                    assert not np.array_equal(want, plain["rows"])
                    sp = g.pcm_split_spectral_pcen_host(trim, cond, s, pc, None, rates)
                    sp0 = g.pcm_split_spectral_host(trim, cond, s, None, rates)
                    assert np.array_equal(g.pcm_split_spectral_pcen_host(trim, cond, s, None, None, rates)["rows"], sp0["rows"])
                    assert np.array_equal(sp["rows"], _run_stage(g, pc, sp0["rows"], sp0["seg_rows"], rates, hop=s.hop_length))
                    if kw["kind"] == "mel_power":  # the post stage behind it
                        full = g.pcm_trim_spectral_pcen_host(trim, cond, s, pc, post, rates)
                        assert full["rc"] == 0 and np.array_equal(full["seg_rows"], plain["seg_rows"])
                        assert np.array_equal(full["rows"], _post_stage(g, post, want, [int(n) for n in plain["seg_rows"]]))
                # resampled to one rate every segment has the same coefficient: the stage alone with that rate
                low = g.pcm_trim_spectral_host(None, None, s, None, rates, 16000)
                on = g.pcm_trim_spectral_pcen_host(None, None, s, pc, None, rates, 16000)
                assert np.array_equal(on["rows"], _run_stage(g, pc, low["rows"], low["seg_rows"], [16000] * S, hop=s.hop_length))
            # a kind whose rows can be negative is refused by name, and so is a bad spec, before anything runs
            bad = _spec()
            bad.eps = 0.0
            for s, p in ((spec_mod.spectral_spec("log_mel", n_fft=400, hop_length=160, n_mels=40), pc),
                         (spec_mod.spectral_spec("stft", n_fft=256, hop_length=64), pc),
                         (spec_mod.spectral_spec("mel_power", n_fft=400, hop_length=160, n_mels=40), bad)):
                with pytest.raises(VsynError) as ei:
                    g.pcm_trim_spectral_pcen_host(None, None, s, p, None, rates)
                assert ei.value.code == 1 and "pcen" in str(ei.value)
        f1b, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        assert np.array_equal(f1, f1b)
        r2 = g.submit_host(b2["packets"], b2["segments"], b2["ys"], b2["residue"], b2["plane_stride"])
        assert r2["rc"] == 0
        outs.append((f1, r2["pcm"], r2["emit_len"]))
        g.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])


E2E = [
    (dict(kind="mel_power", power=1, n_fft=400, hop_length=160, n_mels=40), {}),
    (dict(kind="lin_power", n_fft=512, hop_length=160), {}),
    (dict(kind="mel_power", power=1, n_fft=400, hop_length=160, n_mels=40), dict(trim_db=40)),
    (dict(kind="mel_power", power=1, n_fft=400, hop_length=160, n_mels=40), dict(split_db=40)),
    (dict(kind="mel_power", power=1, n_fft=400, hop_length=160, n_mels=40), dict(delta=1, normalize="mean")),
]


@pytest.fixture(scope="module")
def blobs():
    """The two real fixtures, and the mono one re-headed to 16 kHz so that the rates differ within a call."""
    real = [_ogg("test.stereo44khz"), _ogg("test.mono44khz")]
    return real + [_rehead(real[1], 16000)]


@pytest.mark.parametrize("sr", [None, 16000])
@pytest.mark.parametrize("case", range(len(E2E)))
def test_end_to_end(spec_mod, synth, blobs, case, sr):
    """(7) Measured: worst |d| / (u |Y|) between 0.986 and 0.998 over the ten cases, against the model on the device's own float32
    rows."""
    kw, stages = E2E[case]
    gate_kw = {k: v for k, v in stages.items() if k in ("trim_db", "split_db")}
    post_kw = {k: v for k, v in stages.items() if k in ("delta", "normalize")}
    pk = dict(pcen=True, pcen_scale=2 ** 31)
    ti, si, ti0, si0 = [], [], [], []
    plain = spec_mod.get_spectral_batch(blobs, sr=sr, trim_index=ti0, split_index=si0, **kw, **gate_kw)
    got = spec_mod.get_spectral_batch(blobs, sr=sr, trim_index=ti, split_index=si, **kw, **stages, **pk)
    assert len(got) == len(plain) == 3
    file_rates = [_rate(b) for b in blobs]
    assert file_rates == [44100, 44100, 16000]
    rates = [sr or r for r in file_rates]
    bs = [pm.coefficient(0.4, r, kw["hop_length"]) for r in rates]
    assert (bs[0] == bs[1] != bs[2]) if sr is None else (bs[0] == bs[1] == bs[2])
    pc = _spec(scale=2.0 ** 31)
    worst = 0.0
    for i, (x, y) in enumerate(zip(plain, got)):
        assert x.shape[0] >= 9 and x.dtype == y.dtype == np.float32
        want = _run_stage(synth, pc, x, [x.shape[0]], [rates[i]], hop=kw["hop_length"])
        worst = max(worst, pm.gate(want, x, sr=rates[i], hop_length=kw["hop_length"], **dict(pm.DEFAULTS, scale=2.0 ** 31)))
        if post_kw:
            post, dout, keep = spec_mod.post_spec(x.shape[1], post_kw["delta"], 9, post_kw["normalize"])
            want = _post_stage(synth, post, want, [x.shape[0]])
            assert want.shape[1] == dout
        assert np.array_equal(y, want), (case, sr, i)
    print("end to end %r %r sr %r: worst |d| / (u |Y|) %.3f (gate 2)" % (kw["kind"], stages, sr, worst))
    # the indices are those of the call without the stage
    assert ti == ti0 and len(si) == len(si0) and all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(si, si0))
    if "trim_db" in stages:
        assert all(t is not None for t in ti)
    if "split_db" in stages:
        assert all(s is not None for s in si)


def test_a_refused_kind_never_reaches_the_library_and_a_damaged_file_fails_alone(spec_mod, blobs, monkeypatch):
    kw = dict(kind="mel_power", power=1, n_fft=400, hop_length=160, n_mels=40, pcen=True, pcen_scale=2 ** 31)
    names = [0, 1, 2] * 3
    data = [blobs[i] for i in names]
    bad = bytearray(data[4])
    bad[len(bad) // 2] ^= 0x55  # a page CRC
    data[4] = bytes(bad)
    res = spec_mod.get_spectral_batch(data, errors="return", files_per_submit=4, **kw)
    single = [spec_mod.get_spectral_from_raw_bytes(b, **kw) for b in blobs]
    for i, (n, r) in enumerate(zip(names, res)):
        if i == 4:
            assert isinstance(r, spec_mod.SpectralError) and "file 4" in str(r)
            continue
        assert isinstance(r, np.ndarray) and np.array_equal(r, single[n]), i
    with pytest.raises(spec_mod.SpectralError):
        spec_mod.get_spectral_batch(data, **kw)

    def no_load():
        raise AssertionError("library reached")
    monkeypatch.setattr(spec_mod, "_load", no_load)
    with pytest.raises(spec_mod.SpectralError) as ei:
        spec_mod.get_spectral_batch(blobs, **dict(kw, kind="log_mel"))
    assert "log_mel" in str(ei.value)
