"""HPSS on the device (include/vorbis_synth_hip.h, "HPSS") against the float64 model of tests/hpss_model.py.

The gate, per element and with nothing left out (tests/hpss_model.py gate()): the median output equals the model's as values; the
mask and the component obey |d| <= 2 u |Y| + 2^-126, u = 2^-24: one rounding to float32 and a flushed denormal; the float64
quotient, power and a + b are ratios and sums of non-negative terms and stay far below u, and every decision is exact on float32
medians and one correctly rounded product. Each test prints its worst |d| / (u |Y|) under pytest -s.

(1) the stage alone over D x kernel pairs, ten segments a call, every power x margins x component x output; (2) in place = out of
place; (3) same rows, same bits, wherever the segment lies and whatever its neighbours hold; (4) the non-finite rule; (5) refusals
with the output untouched; (6) the host chain: hpss = NULL is vsyn_pcm_chain_chroma_host, with a spec it is the stage alone on that
entry's rows, then PCEN's and the post stage's on top, and the PCM and the next submit are left alone; (7) get_spectral_batch end to
end."""
import itertools

import numpy as np
import pytest

from tests import hpss_model as hm
from tests.test_gpu_spectral import _ogg, _rate, _rehead

pytestmark = pytest.mark.gpu


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
    return spectral.hpss_spec(kw.get("component", "harmonic"), kw.get("kernel_size", (31, 31)), kw.get("power", 2.0), kw.get("margin", (1.0, 1.0)),
                              kw.get("output", "component"))


def _run_stage(g, hp, x, seg_rows, in_place=False, dim=None):
    """vsyn_spectral_hpss_device over rows x (total, D) float32 split as seg_rows: (total, D) float32. Three rows of NaN behind the
    rows must stay NaN."""
    import torch
    n, D = x.shape
    pad = np.full((3, D), np.nan, np.float32)
    d_in = torch.from_numpy(np.concatenate([np.ascontiguousarray(x), pad])).cuda()
    d_out = d_in if in_place else torch.full((n + 3, D), float("nan"), dtype=torch.float32, device="cuda")
    try:
        g.spectral_hpss_device(hp, D if dim is None else dim, seg_rows, d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    finally:
        torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.isnan(out[n:]).all()  # nothing written past the rows
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy()[:n], x, equal_nan=True)  # the input is read only
    return out[:n]


def _batch(D, seed, seg_rows=hm.SEG_ROWS):
    return [hm.rows(F, D, seed + 17 * i) for i, F in enumerate(seg_rows)]


def _gate_segments(got, segs, HPs, kw):
    worst, o = 0.0, 0
    for X, HP in zip(segs, HPs):
        worst = max(worst, hm.gate(got[o:o + len(X)], X, HP=HP, **kw))
        o += len(X)
    assert o == len(got)
    return worst


@pytest.mark.parametrize("kernel", hm.KERNELS, ids=lambda k: "%dx%d" % k)
@pytest.mark.parametrize("D", hm.DIMS)
def test_stage_alone_against_the_model(synth, D, kernel):
    """(1) Ten segments of 1 .. 200 rows in one call; per (D, kernel pair) every power x margins x component as mask and as component,
    and both medians: 50 calls. Measured on the MI355X, worst |d| / (u |Y|) over the six kernel pairs: D = 1 0.980 to 0.997, 2 0.978 to 0.990, 17 0.989 to
    0.998, 128 0.996 to 1.000, 257 0.996 to 1.000, 1025 0.998 to 1.000: the one rounding to float32; the float64 terms do not show. The
    medians are equal to the model's in every element."""
    segs = _batch(D, 1000 * kernel[0] + D)
    x = np.concatenate(segs)
    HPs = [hm.medians(X, kernel) for X in segs]
    worst = 0.0
    for comp in hm.COMPONENTS:
        kw = dict(component=comp, kernel_size=kernel, output="median")
        _gate_segments(_run_stage(synth, _spec(**kw), x, hm.SEG_ROWS), segs, HPs, kw)  # exact
    for power, margin, comp, output in itertools.product(hm.POWERS, hm.MARGINS, hm.COMPONENTS, ("mask", "component")):
        kw = dict(component=comp, kernel_size=kernel, power=power, margin=margin, output=output)
        got = _run_stage(synth, _spec(**kw), x, hm.SEG_ROWS)
        assert not np.isnan(got).any()
        worst = max(worst, _gate_segments(got, segs, HPs, kw))
    print("stage alone, D %d, kernel %r: worst |d| / (u |Y|) %.3f (gate 2)" % (D, kernel, worst))
    assert worst > 0.5  # the rows are not trivial


@pytest.mark.parametrize("D", [17, 257])
def test_in_place_equals_out_of_place(synth, D):
    """(2)"""
    x = np.concatenate(_batch(D, 7))
    for kw in (dict(kernel_size=(31, 31)), dict(kernel_size=(63, 5), component="percussive", power=0.5, margin=(1.0, 3.0)),
               dict(kernel_size=(5, 63), output="median"), dict(kernel_size=(3, 3), output="mask", power=np.inf)):
        out = _run_stage(synth, _spec(**kw), x, hm.SEG_ROWS)
        assert np.array_equal(_run_stage(synth, _spec(**kw), x, hm.SEG_ROWS, in_place=True), out), (D, kw)


@pytest.mark.parametrize("D", [40, 257])
def test_same_rows_same_bits_wherever_the_segment_lies(synth, D):
    """(3) a segment alone, and the same rows as segment 0, 3 and 7 of a batch of other lengths; then with neighbours full of 1e30,
    which would show in every reflected window if a neighbour's row were read."""
    kw = dict(kernel_size=(63, 31), power=1.0, margin=(2.0, 1.0))
    for F in (3, 33, 130):
        X = hm.rows(F, D, 11 + F)
        alone = _run_stage(synth, _spec(**kw), X, [F])
        lens = [F, 130, 1, F, 0, 63, 70, F, 64]
        offs = np.concatenate([[0], np.cumsum(lens)])
        for fill in (None, 1e30):
            segs = [X if j in (0, 3, 7) else hm.rows(n, D, 31 + j) if fill is None else np.full((n, D), fill, np.float32) for j, n in enumerate(lens)]
            got = _run_stage(synth, _spec(**kw), np.concatenate(segs), lens)
            again = _run_stage(synth, _spec(**kw), np.concatenate(segs), lens)
            assert np.array_equal(got, again)
            for j in (0, 3, 7):
                assert np.array_equal(got[offs[j]:offs[j] + F], alone), (D, F, j, fill)
        hm.gate(alone, X, **kw)
        for comp in hm.COMPONENTS:  # the medians next to the loud neighbours are the segment's own
            kwm = dict(kw, component=comp, output="median")
            got = _run_stage(synth, _spec(**kwm), np.concatenate(segs), lens)
            for j in (0, 3, 7):
                hm.gate(got[offs[j]:offs[j] + F], X, **kwm)


def test_non_finite_rule(synth):
    """(4) a NaN poisons exactly its time window in H and its bin window in P (their union in a soft mask and a component); Inf and -Inf
    sort as numbers and follow the model; every other element keeps the bits it has without them. Measured: worst |d| / (u |Y|) over the finite elements 0.994."""
    F, D, kern = 70, 40, (5, 7)
    X0 = hm.rows(F, D, 5)
    X = X0.copy()
    X[20, 10] = np.nan
    X[69, 39] = np.nan  # a corner: the windows reflect
    X[40, 4] = np.inf
    X[41, 4] = np.inf
    X[42, 4] = np.inf  # three of five: the time median of (41, 4) is Inf
    X[50, 20] = -np.inf
    inH, inP = np.zeros((F, D), bool), np.zeros((F, D), bool)
    inH[18:23, 10] = inH[67:70, 39] = True
    inP[20, 7:14] = inP[69, 36:40] = True
    worst = 0.0
    for comp in hm.COMPONENTS:
        kw = dict(component=comp, kernel_size=kern, output="median")
        got = _run_stage(synth, _spec(**kw), X, [F])
        assert np.array_equal(np.isnan(got), inH if comp == "harmonic" else inP)
        hm.gate(got, X, **kw)
        clean = _run_stage(synth, _spec(**kw), X0, [F])
        far = np.ones((F, D), bool)
        if comp == "harmonic":
            far[:, [10, 39, 4, 20]] = False
        else:
            far[[20, 69, 40, 41, 42, 50]] = False
        assert np.array_equal(got[far], clean[far])  # everything whose window holds none of them keeps its bits
    assert np.isposinf(_run_stage(synth, _spec(kernel_size=kern, output="median"), X, [F])[41, 4])
    for power, margin, comp, output in itertools.product(hm.POWERS, hm.MARGINS[:2], hm.COMPONENTS, ("mask", "component")):
        kw = dict(component=comp, kernel_size=kern, power=power, margin=margin, output=output)
        got = _run_stage(synth, _spec(**kw), X, [F])
        worst = max(worst, hm.gate(got, X, **kw))
        if np.isfinite(power):
            want_nan = inH | inP
            assert np.isnan(got[want_nan]).all()
            rest = np.isnan(got) & ~want_nan  # only Inf / Inf and Inf * 0 may add NaNs, and only in the Infs' own windows
            assert not rest[:, [c for c in range(D) if c not in (4, 20)]][[r for r in range(F) if r not in (40, 41, 42, 50)]].any()
    print("non-finite rule: worst |d| / (u |Y|) over the finite elements %.3f (gate 2)" % worst)


def test_stage_refuses_bad_arguments_and_writes_nothing(synth):
    """(5)"""
    import torch
    from parseoggvorbis_amd.binding import VsynError
    x = hm.rows(20, 8, 1)
    cases = []
    for field, values in (("kh", (0, 2, 30, 65, 64)), ("kp", (0, 4, 65, 1 << 31)), ("component", (2, 7)), ("output", (3, 9)),
                          ("power", (0.0, -1.0, np.nan, -np.inf)), ("margin_h", (0.5, np.inf, np.nan, -1.0)), ("margin_p", (0.99, np.inf, np.nan))):
        for v in values:
            hp = _spec()
            setattr(hp, field, v)
            cases.append((hp, 8))
    cases.append((_spec(), 0))
    cases.append((None, 8))
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.full((20, 8), float("nan"), dtype=torch.float32, device="cuda")
    for hp, dim in cases:
        with pytest.raises(VsynError) as ei:
            synth.spectral_hpss_device(hp, dim, [20], d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert ei.value.code == 1, str(ei.value)  # VSYN_ERR_INVALID
    torch.cuda.synchronize()
    assert np.isnan(d_out.cpu().numpy()).all()
    synth.spectral_hpss_device(_spec(power=np.inf), 8, [20], d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), _run_stage(synth, _spec(power=np.inf), x, [20]))


def _pcen_stage(g, pc, x, seg_rows, rates, hop):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    g.spectral_pcen_device(pc, x.shape[1], seg_rows, rates, hop, d.data_ptr(), d.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d.cpu().numpy()


def _post_stage(g, post, x, seg_rows):
    import torch
    D = x.shape[1]
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.full((x.shape[0], D * (1 + post.order)), float("nan"), dtype=torch.float32, device="cuda")
    g.spectral_post_device(post, D, seg_rows, d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def test_host_chain(spec_mod):
    """(6)"""
    from parseoggvorbis_amd.binding import PcmCond, PcmTrim, SpectralPost, Synth, VsynError, VSYN_PCM_F32
    from tests.workloads import fixture_like_spec, synth_batch
    spec = fixture_like_spec(2)
    b1 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=11)
    b2 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=12)
    S = len(b1["segments"])
    rates = [44100, 22050, 44100][:S] + [44100] * max(0, S - 3)
    post = SpectralPost(2, 3, 2, 0, 1e-5, None, None)  # delta 2 over width 3, mean_var
    pc = spec_mod.pcen_spec(scale=2.0 ** 31)
    hp = _spec(kernel_size=(17, 9), margin=(2.0, 1.0))
    outs = []
    for with_hpss in (False, True):
        g = Synth(spec, device=0, max_streams=4)
        r1 = g.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"], flags=4)  # KEEP_PCM
        assert r1["rc"] == 0
        f1, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        if with_hpss:
            for kw in (dict(kind="mel_power", power=1, n_fft=400, hop_length=160, n_mels=40), dict(kind="lin_power", n_fft=256, hop_length=64)):
                s = spec_mod.spectral_spec(**kw)
                for gate, is_split, cond in ((None, 0, None), (PcmTrim(256, 64, 40.0), 0, PcmCond(1, 0, 0.0)), (PcmTrim(256, 64, 40.0), 1, PcmCond(1, 0, 0.0))):
                    plain = g.pcm_chain_chroma_host(gate, is_split, None, cond, s, None, None, None, rates)
                    off = g.pcm_chain_hpss_host(gate, is_split, None, cond, s, None, None, None, None, rates)
                    assert off["rc"] == 0 and plain["rows"].shape[0] > 0
                    for k in ("rows", "seg_rows", "bounds", "frames", "counts", "peaks", "refs"):
                        assert np.array_equal(off[k], plain[k]), k
                    nrows = [int(n) for n in plain["seg_rows"]]
                    on = g.pcm_chain_hpss_host(gate, is_split, None, cond, s, None, hp, None, None, rates)
                    want = _run_stage(g, hp, plain["rows"], nrows)
                    assert on["rc"] == 0 and np.array_equal(on["seg_rows"], plain["seg_rows"]) and np.array_equal(on["rows"], want)
                    assert np.array_equal(on["bounds"], plain["bounds"]) and not np.array_equal(want, plain["rows"])
                    both = g.pcm_chain_hpss_host(gate, is_split, None, cond, s, None, hp, pc, None, rates)
                    want_pc = _pcen_stage(g, pc, want, nrows, rates, s.hop_length)
                    assert both["rc"] == 0 and np.array_equal(both["rows"], want_pc)
                    # PCEN alone through the new entry is PCEN through the old one
                    assert np.array_equal(g.pcm_chain_hpss_host(gate, is_split, None, cond, s, None, None, pc, None, rates)["rows"],
                                          g.pcm_chain_chroma_host(gate, is_split, None, cond, s, None, pc, None, rates)["rows"])
                    if kw["kind"] == "mel_power":  # the post stage behind both
                        full = g.pcm_chain_hpss_host(gate, is_split, None, cond, s, None, hp, pc, post, rates)
                        assert full["rc"] == 0 and np.array_equal(full["seg_rows"], plain["seg_rows"])
                        assert np.array_equal(full["rows"], _post_stage(g, post, want_pc, nrows))
            # refused by name before anything runs: another kind, PCEN on the mask or the median, a bad spec
            bad = _spec()
            bad.kh = 30
            mel = spec_mod.spectral_spec("mel_power", n_fft=400, hop_length=160, n_mels=40)
            for s, h, p, word in ((spec_mod.spectral_spec("log_mel", n_fft=400, hop_length=160, n_mels=40), hp, None, "hpss"),
                                  (spec_mod.spectral_spec("stft", n_fft=256, hop_length=64), hp, None, "hpss"),
                                  (spec_mod.spectral_spec("lin_db", n_fft=256, hop_length=64), hp, None, "hpss"),
                                  (mel, _spec(output="mask"), pc, "mask"), (mel, _spec(output="median"), pc, "median"), (mel, bad, None, "hpss")):
                with pytest.raises(VsynError) as ei:
                    g.pcm_chain_hpss_host(None, 0, None, None, s, None, h, p, None, rates)
                assert ei.value.code == 1 and word in str(ei.value)
        f1b, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        assert np.array_equal(f1, f1b)
        r2 = g.submit_host(b2["packets"], b2["segments"], b2["ys"], b2["residue"], b2["plane_stride"])
        assert r2["rc"] == 0
        outs.append((f1, r2["pcm"], r2["emit_len"]))
        g.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])


MEL = dict(kind="mel_power", power=1, n_fft=400, hop_length=160, n_mels=40)
E2E = [
    (MEL, {}, dict(hpss="harmonic")),
    (dict(kind="lin_power", n_fft=512, hop_length=160), {}, dict(hpss="percussive", hpss_kernel_size=(17, 31), hpss_margin=(1.0, 2.0))),
    (MEL, dict(trim_db=40), dict(hpss="percussive", hpss_power=1.0)),
    (MEL, dict(pcen=True, pcen_scale=2 ** 31), dict(hpss="harmonic", hpss_kernel_size=63)),
    (MEL, dict(delta=1, normalize="mean"), dict(hpss="harmonic", hpss_margin=3.0)),
    (MEL, {}, dict(hpss="harmonic", hpss_output="mask", hpss_power=np.inf)),
    (dict(kind="lin_power", n_fft=512, hop_length=160), {}, dict(hpss="percussive", hpss_output="median", hpss_kernel_size=(5, 63))),
]


@pytest.fixture(scope="module")
def blobs():
    """The two real fixtures, and the mono one re-headed to 16 kHz so that the rates differ within a call."""
    real = [_ogg("test.stereo44khz"), _ogg("test.mono44khz")]
    return real + [_rehead(real[1], 16000)]


def _model_kw(hk):
    ks, mg = hk.get("hpss_kernel_size", 31), hk.get("hpss_margin", 1.0)
    return dict(component=hk["hpss"], kernel_size=ks if isinstance(ks, tuple) else (ks, ks), power=hk.get("hpss_power", 2.0),
                margin=mg if isinstance(mg, tuple) else (mg, mg), output=hk.get("hpss_output", "component"))


@pytest.mark.parametrize("sr", [None, 16000])
@pytest.mark.parametrize("case", range(len(E2E)))
def test_end_to_end(spec_mod, synth, blobs, case, sr):
    """(7) get_spectral_batch(hpss=...) on the golden Ogg files against the model on the rows of the same call without hpss; PCEN and
    the post stage on top are the device's own stages on those rows. Measured: worst |d| / (u |Y|) between 0.990 and 0.999 over the ten
    component cases; the hard mask and the median are exact (0)."""
    kw, stages, hk = E2E[case]
    gate_kw = {k: v for k, v in stages.items() if k in ("trim_db",)}
    post_kw = {k: v for k, v in stages.items() if k in ("delta", "normalize")}
    ti, ti0 = [], []
    plain = spec_mod.get_spectral_batch(blobs, sr=sr, trim_index=ti0, **kw, **gate_kw)
    got = spec_mod.get_spectral_batch(blobs, sr=sr, trim_index=ti, **kw, **stages, **hk)
    assert len(got) == len(plain) == 3
    rates = [sr or _rate(b) for b in blobs]
    mk = _model_kw(hk)
    worst = 0.0
    for i, (x, y) in enumerate(zip(plain, got)):
        assert x.shape[0] >= 9 and x.dtype == y.dtype == np.float32
        want = _run_stage(synth, _spec(**mk), x, [x.shape[0]])
        worst = max(worst, hm.gate(want, x, **mk))
        if stages.get("pcen"):
            want = _pcen_stage(synth, spec_mod.pcen_spec(scale=2.0 ** 31), want, [x.shape[0]], [rates[i]], kw["hop_length"])
        if post_kw:
            post, dout, keep = spec_mod.post_spec(x.shape[1], post_kw["delta"], 9, post_kw["normalize"])
            want = _post_stage(synth, post, want, [x.shape[0]])
            assert want.shape[1] == dout
        assert np.array_equal(y, want, equal_nan=True), (case, sr, i)
        assert not np.array_equal(y[:, :x.shape[1]], x)
    print("end to end %r %r %r sr %r: worst |d| / (u |Y|) %.3f (gate 2)" % (kw["kind"], stages, hk, sr, worst))
    assert ti == ti0  # the indices are those of the call without the stage
    if "trim_db" in stages:
        assert all(t is not None for t in ti)


def test_a_damaged_file_fails_alone_and_hpss_none_is_the_call_without_it(spec_mod, blobs):
    kw = dict(MEL, hpss="percussive", hpss_kernel_size=(9, 5))
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
    off = spec_mod.get_spectral_batch(blobs, **dict(kw, hpss=None))
    for a, b in zip(off, spec_mod.get_spectral_batch(blobs, **MEL)):
        assert np.array_equal(a, b)
