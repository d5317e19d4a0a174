"""The constant-Q stage on the GPU (vsyn_cqt_device, vsyn_pcm_cqt_host, ogg_vorbis_cqt_corpus, get_cqt_batch, get_chroma_cqt_batch)
against the float64 model of tests/cqt_model.py: |device - model| <= the model's derived bound for every value, nothing excluded.
The shapes are placed from vsyn_cqt_tile's three numbers (frames per workgroup FT, samples per chunk K, bins per workgroup BPW), not
from constants: the smallest at which the kernel can still go wrong. Each test prints its worst |d| / bound."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import cqt_model as m
from tests.test_gpu_condition import _bits, synth  # noqa: F401
from tests.test_gpu_spectral import _ogg, _rate
from tests.test_gpu_trim import _batch

pytestmark = pytest.mark.gpu


def _spec(**kw):
    """(the C spec, the model's spec) of the same arguments."""
    from parseoggvorbis_amd import cqt
    return cqt.cqt_spec(**kw), m.spec(**kw)


@functools.lru_cache(maxsize=1)
def _tile():
    from parseoggvorbis_amd import binding
    return binding.cqt_tile(_spec()[0], 22050)


def _signal(Cn, T, sr, seed):
    """(C, T) float32: three tones between 100 Hz and sr / 3 with a slow tremolo, and noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64) / sr
    x = np.zeros((Cn, T))
    for c in range(Cn):
        for f in rng.uniform(100.0, sr / 3.0, 3):
            x[c] += 0.2 * np.cos(2.0 * np.pi * f * t + rng.uniform(0, 6.28)) * (1.0 + 0.3 * np.cos(2.0 * np.pi * 3.0 * t))
        x[c] += 0.1 * rng.standard_normal(T)
    return x.astype(np.float32)


def _run(g, spec, x, frames, rates, in_off=0, extra_rows=3):
    """vsyn_cqt_device over x (S, C, plane) float32 with frames [S] and rates [S]: dict(rows: a list of (F, dim) float32 arrays,
    off [S+1], refused [S]). Asserts that nothing behind the last row was written and that the offsets are the host's counts."""
    import torch
    S, Cn, plane = x.shape
    dim = int(g.lib.vsyn_cqt_dim(C.byref(spec)))
    buf = torch.zeros(x.size + 8, dtype=torch.float32, device="cuda")
    buf[in_off:in_off + x.size].copy_(torch.from_numpy(np.ascontiguousarray(x).ravel()))
    d_frames = torch.from_numpy(np.asarray(frames, np.int64).astype(np.uint32).view(np.int32)).cuda()
    counts = [int(g.lib.vsyn_cqt_num_frames(C.byref(spec), min(int(t), plane))) if r else 0 for t, r in zip(frames, rates)]
    cap = sum(counts) + extra_rows
    d_rows = torch.full((cap, dim), -7.0, dtype=torch.float32, device="cuda")
    d_off = torch.full((S + 1,), -1, dtype=torch.int64, device="cuda")
    d_ref = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    g.cqt_device(spec, rates, buf.data_ptr() + 4 * in_off, plane, Cn, d_frames.data_ptr(), d_rows.data_ptr(), d_off.data_ptr(),
                 d_ref.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rows, off = d_rows.cpu().numpy(), d_off.cpu().numpy()
    assert off[0] == 0 and list(np.diff(off)) == counts, (list(np.diff(off)), counts)
    assert (rows[off[-1]:] == -7.0).all()
    return dict(rows=[rows[off[i]:off[i + 1]] for i in range(S)], off=off, refused=d_ref.cpu().numpy())


def _one(g, kw, sr, T, Cn=1, seed=0, x=None):
    """One segment alone under kw against the model: the worst ratio."""
    spec, msp = _spec(**kw)
    x = _signal(Cn, T, sr, seed) if x is None else x
    xs, frames = _batch([x], False)
    got = _run(g, spec, xs, frames, [sr])
    assert list(got["refused"]) == [0]
    assert got["rows"][0].shape[0] == m.num_frames(msp, T)
    return m.check(got["rows"][0], x, msp, sr, _tile()[1], (kw, sr, T, Cn))


def _grow(kw, sr, above):
    """kw with filter_scale raised until the model's L_0 exceeds `above`."""
    kw = dict(kw)
    while m.lengths(m.spec(**kw), sr)[1][0] <= above:
        kw["filter_scale"] = kw.get("filter_scale", 1.0) * 1.25
    return kw


def test_lengths_against_the_wave_and_the_chunk(synth):
    """Supports below one wave, between one and two and above two; the even L; L_0 at K - 1, K and K + 1 (bpo = 1 with
    filter_scale = 3 / 5 makes Q = 1 and N_0 = sr / fmin exactly); L_0 above two chunks; librosa's defaults (L_0 = 11685)."""
    FT, K, BPW = _tile()
    worst = 0.0
    wave = dict(fmin=250.0, n_bins=9, bins_per_octave=3, hop_length=64)
    L = m.lengths(m.spec(**wave), 8000)[1]
    assert min(L) < 64 < sorted(L)[-3] < 128 < max(L)
    worst = max(worst, _one(synth, wave, 8000, 3000, seed=1))
    even = dict(fmin=100.0, n_bins=3, bins_per_octave=1, hop_length=50)
    assert m.lengths(m.spec(**even), 12000)[1] == [200, 100, 50]
    worst = max(worst, _one(synth, even, 12000, 2000, seed=2))
    for L0 in (K - 1, K, K + 1):
        kw = dict(fmin=8192.0 / L0, n_bins=2, bins_per_octave=1, filter_scale=3.0 / 5.0, hop_length=300)
        assert m.lengths(m.spec(**kw), 8192)[1][0] == L0
        worst = max(worst, _one(synth, kw, 8192, 4000, seed=L0))
    two = _grow(dict(fmin=60.0, n_bins=8, bins_per_octave=6, hop_length=500), 16000, 2 * K)
    assert m.lengths(m.spec(**two), 16000)[1][0] > 2 * K
    worst = max(worst, _one(synth, two, 16000, 6000, seed=3))
    dflt = dict(hop_length=4096)
    assert m.lengths(m.spec(**dflt), 22050)[1][0] == 11685
    worst = max(worst, _one(synth, dflt, 22050, 12000, seed=4))
    print("constant-Q lengths: worst |d| / bound %.4f" % worst)
    assert worst < 1.0


def test_bin_counts(synth):
    """n_bins 1, BPW - 1, BPW, BPW + 1 and 256 (a high bpo and fmin at 16 kHz, so that the supports stay short and step 10 passes)."""
    FT, K, BPW = _tile()
    worst = 0.0
    for nb in sorted({1, BPW - 1, BPW, BPW + 1}):
        if nb >= 1:
            worst = max(worst, _one(synth, dict(fmin=300.0, n_bins=nb, bins_per_octave=4, hop_length=128), 8000, 1500, seed=nb))
    big = dict(fmin=1900.0, n_bins=256, bins_per_octave=128, hop_length=700)
    assert not m.rate_refused(m.spec(**big), 16000)
    worst = max(worst, _one(synth, big, 16000, 2500, seed=9))
    print("constant-Q bin counts: worst |d| / bound %.4f" % worst)
    assert worst < 1.0


def test_frame_counts_and_hops(synth):
    """T in {1, hop - 1, hop, hop + 1}; T < L_0 (every sum clipped on both sides); F in FT - 1, FT, FT + 1; hop in {1, 7, 64}; a hop
    above L_0, and one above the chunk as well (frames staged back to back, the samples between them never read)."""
    FT, K, BPW = _tile()
    worst = 0.0
    base = dict(fmin=200.0, n_bins=6, bins_per_octave=3)
    L0 = m.lengths(m.spec(**base), 8000)[1][0]
    for T in (1, 63, 64, 65):
        worst = max(worst, _one(synth, dict(base, hop_length=64), 8000, T, seed=T))
    assert L0 > 100
    worst = max(worst, _one(synth, dict(base, hop_length=16), 8000, 100, seed=5))
    for F in (FT - 1, FT, FT + 1):
        worst = max(worst, _one(synth, dict(base, hop_length=64), 8000, (F - 1) * 64 + 10, Cn=2, seed=F))
    for hop, T in ((1, 2 * FT + 3), (7, 400), (64, 1000)):
        worst = max(worst, _one(synth, dict(base, hop_length=hop), 8000, T, seed=hop))
    assert L0 < 400 < K
    worst = max(worst, _one(synth, dict(base, hop_length=400), 8000, 400 * (FT + 2) + 7, seed=6))
    worst = max(worst, _one(synth, dict(base, hop_length=K + 77), 8000, (K + 77) * (FT + 1) + 300, seed=7))
    long = _grow(dict(fmin=60.0, n_bins=5, bins_per_octave=6), 16000, 2 * K)
    worst = max(worst, _one(synth, dict(long, hop_length=K + 500), 16000, (K + 500) * 3 + 5, seed=8))
    print("constant-Q frame counts and hops: worst |d| / bound %.4f" % worst)
    assert worst < 1.0


OPTIONS = [dict(norm=1), dict(norm=2), dict(norm=None), dict(scale=False), dict(power=2), dict(gamma=25.0), dict(tuning=0.31),
           dict(filter_scale=0.7), dict(filter_scale=1.9, gamma=4.0, norm=2, scale=False, power=2), dict(output="complex"),
           dict(output="complex", scale=False, norm=None)]
OPTIONS += [dict(output="chroma", n_chroma=12, chroma_norm=cn, base_c=bc) for cn in (np.inf, 1, 2, None) for bc in (True, False)]
OPTIONS += [dict(output="chroma", n_chroma=6, bins_per_octave=12), dict(output="tonnetz"), dict(output="tonnetz", base_c=False, chroma_norm=2)]


def test_every_option(synth):
    """norm, scale, power, gamma, tuning, filter_scale, the complex output (both components under the bound), chroma with each norm
    and base_c both ways, tonnetz; two channels, so that the downmix term is in every bound."""
    worst = 0.0
    for i, opt in enumerate(OPTIONS):
        kw = dict(dict(fmin=110.0, n_bins=30, bins_per_octave=12, hop_length=256), **opt)
        worst = max(worst, _one(synth, kw, 11025, 2600, Cn=2, seed=40 + i))
    kw = dict(fmin=65.0, n_bins=72, bins_per_octave=36, hop_length=512, output="chroma")
    worst = max(worst, _one(synth, kw, 8000, 3000, seed=70))
    print("constant-Q options: worst |d| / bound %.4f" % worst)
    assert worst < 1.0


def _mixed_batch():
    kw = dict(fmin=150.0, n_bins=13, bins_per_octave=4, hop_length=200)
    msp = m.spec(**kw)
    rates = [8000, 16000, 0, 11025, 2000, 8000, 16000]
    assert [m.rate_refused(msp, r) for r in rates if r] == [False, False, False, True, False, False]
    Ts = [3001, 2500, 1800, 2999, 2200, 1234, 3100]
    segs = [_signal(2, T, r or 8000, 100 + i) for i, (T, r) in enumerate(zip(Ts, rates))]
    return kw, rates, segs


def test_a_batch_of_rates_skips_and_refusals(synth):
    """Two channels at a non-zero plane offset and an odd stride; several rates in one call (the per-rate tables and the rate
    index); a rate of 0, a segment with an Inf (step 9) and one whose rate step 10 refuses in the middle: refused = 0 / 1 / 2 as
    specified, the refused rows NaN, the neighbours' rows those of a batch without the bad sample, bit for bit, and under the bound."""
    kw, rates, segs = _mixed_batch()
    spec, msp = _spec(**kw)
    x, frames = _batch(segs, True)
    clean = _run(synth, spec, x, frames, rates, in_off=3)
    assert list(clean["refused"]) == [0, 0, 0, 0, 2, 0, 0]
    bad = x.copy()
    bad[3, 1, 2998] = np.inf
    bad[4, 0, 5] = np.nan  # (the rate refusal wins: nothing of the segment is read)
    got = _run(synth, spec, bad, frames, rates, in_off=3)
    assert list(got["refused"]) == [0, 0, 0, 1, 2, 0, 0]
    worst = 0.0
    for i, (seg, r) in enumerate(zip(segs, rates)):
        if r == 0:
            assert got["rows"][i].shape[0] == 0
            continue
        assert got["rows"][i].shape[0] == 1 + seg.shape[1] // 200
        if i in (3, 4):
            assert np.isnan(got["rows"][i]).all()
        else:
            assert np.array_equal(_bits(got["rows"][i]), _bits(clean["rows"][i])), i
        if i != 4:
            worst = max(worst, m.check(clean["rows"][i], seg, msp, r, _tile()[1], ("batch", i)))
        else:
            assert np.isnan(clean["rows"][i]).all()
    for value, t in ((-np.inf, 0), (np.nan, 1233)):  # the first and the last sample of a segment
        bad = x.copy()
        bad[5, 0, t] = value
        got = _run(synth, spec, bad, frames, rates)
        assert list(got["refused"]) == [0, 0, 0, 0, 2, 1, 0] and np.isnan(got["rows"][5]).all()
        assert np.array_equal(_bits(got["rows"][6]), _bits(clean["rows"][6])) and np.array_equal(_bits(got["rows"][3]), _bits(clean["rows"][3]))
    print("constant-Q batch: worst |d| / bound %.4f" % worst)
    assert worst < 1.0


def test_same_bits(synth):
    """A segment alone, in slot 0, in the last slot and at other alignments gives identical rows; a second call on the same handle
    (the wavelet table is not rebuilt) gives identical rows; so does a call after another spec has replaced the table."""
    kw, rates, segs = _mixed_batch()
    for out in ("magnitude", "complex", "chroma"):
        kw2 = dict(kw, output=out) if out != "chroma" else dict(kw, output=out, n_chroma=4)
        spec = _spec(**kw2)[0]
        x, frames = _batch(segs, False)
        base = _run(synth, spec, x, frames, rates)
        again = _run(synth, spec, x, frames, rates)
        assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(base["rows"], again["rows"]))
        order = list(range(len(segs)))[::-1]
        mixed = _run(synth, spec, x[order], [frames[j] for j in order], [rates[j] for j in order])
        for j, src in enumerate(order):
            assert np.array_equal(_bits(mixed["rows"][j]), _bits(base["rows"][src])), (out, src)
        for src in (0, 3, 6):
            alone = _run(synth, spec, x[src:src + 1], frames[src:src + 1], rates[src:src + 1])
            assert np.array_equal(_bits(alone["rows"][0]), _bits(base["rows"][src])), (out, src)
        odd = np.zeros((x.shape[0], 2, x.shape[2] + 3), np.float32)
        odd[:, :, :x.shape[2]] = x
        for off in (0, 1, 2, 3):
            shifted = _run(synth, spec, odd, frames, rates, off)
            assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(base["rows"], shifted["rows"])), (out, off)
        _run(synth, _spec(fmin=300.0, n_bins=3, bins_per_octave=2, hop_length=100)[0], x, frames, rates)
        back = _run(synth, spec, x, frames, rates)
        assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(base["rows"], back["rows"]))


def hann_image_bound(L, nu):
    """|sum_j w[j] e^(-2 pi i nu j)| / sum_j w[j] for the periodic Hann of L samples at nu cycles per sample, from its three Dirichlet
    kernels, each at most 1 / |sin(pi x)|."""
    d = lambda v: 1.0 / abs(math.sin(math.pi * v))
    return (0.5 * d(nu) + 0.25 * d(nu - 1.0 / L) + 0.25 * d(nu + 1.0 / L)) / (L / 2.0)


def test_closed_form_on_the_device(synth):
    """A cosine of amplitude A at exactly f_k: every frame whose support lies inside the signal has |C[t][k]| = sqrt(N_k) A / 2 up to
    the image term A / 2 |W(2 f_k / sr)| / sum w, bounded analytically, plus the model's rounding bound. Per bin."""
    A, sr, T = 0.7, 8000, 2500
    kw = dict(fmin=250.0, n_bins=9, bins_per_octave=3, hop_length=100)
    spec, msp = _spec(**kw)
    N, L, h = m.lengths(msp, sr)
    worst = 0.0
    for k, f in enumerate(m.frequencies(msp)):
        x = (A * np.cos(2.0 * np.pi * f * np.arange(T) / sr + 0.4))[None, :].astype(np.float32)
        xs, frames = _batch([x], False)
        rows = _run(synth, spec, xs, frames, [sr])["rows"][0]
        tol = m.bound(x, msp, sr, _tile()[1])
        inside = [t for t in range(rows.shape[0]) if t * 100 - h[k] >= 0 and t * 100 - h[k] + L[k] <= T]
        assert len(inside) >= 5
        want = math.sqrt(N[k]) * A / 2.0
        image = want * hann_image_bound(L[k], 2.0 * f / sr)
        quant = math.sqrt(N[k]) * 2.0 ** -24 * A  # the float32 rounding of the samples themselves, through sum |b| = 1
        for t in inside:
            d = abs(float(rows[t, k]) - want)
            worst = max(worst, d / (image + tol[t, k] + quant))
            assert d <= image + tol[t, k] + quant, (k, t, d, image, tol[t, k])
    print("constant-Q closed form: worst |d| / (image + bound) %.4f" % worst)


E2E_FILES = ["test.mono44khz", "synth_03", "test.stereo44khz"]


@pytest.mark.parametrize("sr", [None, 16000])
def test_end_to_end_against_the_model(sr):
    """get_cqt_batch (magnitude and complex) and get_chroma_cqt_batch (chroma and tonnetz) on golden files against the model on what
    get_pcm_batch(mono=True, sr=sr) returns, with a large hop so that it takes seconds; a damaged file fails alone; the one-file
    forms are bit-equal."""
    import torch
    assert torch.cuda.is_available()
    from parseoggvorbis_amd import cqt, pcm
    blobs = [_ogg(n) for n in E2E_FILES]
    planes = pcm.get_pcm_batch(blobs, sr=sr, mono=True)
    broken = blobs[0][:len(blobs[0]) // 8]
    K = _tile()[1]
    worst = 0.0
    runs = [(cqt.get_cqt_batch, cqt.get_cqt_from_raw_bytes, dict(fmin=110.0, n_bins=24, bins_per_octave=6, hop_length=8192), {}),
            (cqt.get_cqt_batch, cqt.get_cqt_from_raw_bytes, dict(fmin=110.0, n_bins=24, bins_per_octave=6, hop_length=8192, output="complex"), {}),
            (cqt.get_chroma_cqt_batch, cqt.get_chroma_cqt_from_raw_bytes, dict(fmin=65.0, n_octaves=3, bins_per_octave=12, hop_length=8192),
             dict(output="chroma")),
            (cqt.get_chroma_cqt_batch, cqt.get_chroma_cqt_from_raw_bytes,
             dict(fmin=65.0, n_octaves=2, bins_per_octave=24, hop_length=8192, tonnetz=True, base_c=False), dict(output="tonnetz"))]
    for batch, single, kw, extra in runs:
        got = batch(list(blobs) + [broken], sr=sr, errors="return", **kw)
        assert isinstance(got[-1], cqt.CqtError) and not any(isinstance(r, Exception) for r in got[:-1])
        with pytest.raises(cqt.CqtError, match="file %d" % len(blobs)):
            batch(list(blobs) + [broken], sr=sr, **kw)
        one = single(blobs[1], sr=sr, **kw)
        assert one[1] == got[1][1] and np.array_equal(_bits(one[0].view(np.float32)), _bits(got[1][0].view(np.float32)))
        mk = {k: v for k, v in kw.items() if k not in ("n_octaves", "tonnetz")}
        if "n_octaves" in kw:
            mk["n_bins"] = kw["n_octaves"] * kw["bins_per_octave"]
        msp = m.spec(**dict(mk, **extra))
        for name, data, (y, r), (rows, rate) in zip(E2E_FILES, blobs, planes, got):
            assert rate == r == (sr or _rate(data))
            if kw.get("output") == "complex":
                assert rows.dtype == np.complex64 and rows.shape[1] == 24
                rows = rows.view(np.float32)
            worst = max(worst, m.check(rows, y, msp, rate, K, (name, sr, kw)))
    print("constant-Q end to end (sr %s): worst |d| / bound %.4f" % (sr, worst))
    assert worst < 1.0


def test_refusals_end_to_end():
    """A file at whose rate step 10 refuses the spec (a fixture re-headed to 16 kHz beside the original) fails alone and its error
    says so; resampled to a rate that step 10 refuses, every file does."""
    from parseoggvorbis_amd import cqt
    from tests.test_gpu_spectral import _rehead
    blobs = [_ogg("synth_03"), _rehead(_ogg("synth_03"), 16000), _ogg("test.mono44khz")]
    kw = dict(fmin=4000.0, n_bins=13, bins_per_octave=12, hop_length=8192)
    msp = m.spec(**kw)
    assert [m.rate_refused(msp, _rate(b)) for b in blobs] == [False, True, False]
    got = cqt.get_cqt_batch(blobs, errors="return", **kw)
    assert isinstance(got[1], cqt.CqtError) and "Nyquist" in str(got[1]) and "16000" in str(got[1])
    assert not isinstance(got[0], Exception) and not isinstance(got[2], Exception)
    alone = cqt.get_cqt_from_raw_bytes(blobs[0], **kw)
    assert np.array_equal(_bits(alone[0]), _bits(got[0][0]))
    with pytest.raises(cqt.CqtError, match="file 1"):
        cqt.get_cqt_batch(blobs, **kw)
    got = cqt.get_cqt_batch(blobs, errors="return", sr=8000, **kw)
    assert all(isinstance(r, cqt.CqtError) and "Nyquist" in str(r) for r in got)


BAD_SPECS = [dict(n_bins=0), dict(n_bins=257), dict(bins_per_octave=0), dict(bins_per_octave=257), dict(hop_length=0), dict(fmin=0.0),
             dict(fmin=-1.0), dict(fmin=float("inf")), dict(fmin=float("nan")), dict(filter_scale=0.0), dict(filter_scale=float("inf")),
             dict(gamma=-1e-9), dict(gamma=float("nan")), dict(tuning=float("inf")), dict(power=0), dict(power=3), dict(norm=3),
             dict(output=0), dict(output=5), dict(options=4), dict(reserved=1), dict(output=3, n_chroma=0), dict(output=3, n_chroma=257),
             dict(output=3, n_chroma=5), dict(output=4, n_chroma=12, chroma_norm=4)]


def _raw(**kw):
    from parseoggvorbis_amd.binding import CqtSpec
    d = dict(n_bins=12, bins_per_octave=12, hop_length=64, options=1, output=1, power=1, norm=1, n_chroma=12, chroma_norm=3, reserved=0,
             fmin=200.0, tuning=0.0, filter_scale=1.0, gamma=0.0)
    d.update(kw)
    return CqtSpec(**d)


def test_bad_specs_are_refused_with_nothing_launched(synth):
    """Each invalid spec of step 11, channels = 0 and NULL rates: VSYN_ERR_INVALID from both entry points and nothing written; on
    the device the caps are tested on the accepted side only (tests/test_cqt_cpu.py has both sides)."""
    import torch
    from parseoggvorbis_amd.binding import Status, Synth, VsynError
    from tests.workloads import fixture_like_spec, synth_batch
    t = torch.full((4096,), 5.0, dtype=torch.float32, device="cuda")
    f = torch.full((8,), 64, dtype=torch.int32, device="cuda")
    o = torch.full((64,), 9, dtype=torch.int32, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return (t.cpu().numpy() == 5.0).all() and (o.cpu().numpy() == 9).all()
    for kw in BAD_SPECS:
        with pytest.raises(VsynError) as ei:
            synth.cqt_device(_raw(**kw), (8000,), t.data_ptr(), 64, 2, f.data_ptr(), t.data_ptr() + 2048, o.data_ptr(), o.data_ptr() + 128)
        assert ei.value.code == 1 and untouched(), kw
        assert synth.lib.vsyn_cqt_dim(C.byref(_raw(**kw))) == 0 and synth.lib.vsyn_cqt_num_frames(C.byref(_raw(**kw)), 1000) == 0
    for kw in (dict(channels=0), dict(rates=None)):
        err = C.c_char_p()
        rates = np.array([8000], np.uint32)
        rc = synth.lib.vsyn_cqt_device(synth.h, C.byref(_raw()), 1, None if "rates" in kw else rates.ctypes.data, t.data_ptr(), 64,
                                       kw.get("channels", 2), f.data_ptr(), t.data_ptr() + 2048, o.data_ptr(), o.data_ptr() + 128, None, C.byref(err))
        assert rc == 1 and err.value and untouched(), kw
    assert synth.lib.vsyn_cqt_num_frames(C.byref(_raw()), 1000) == 16 and synth.lib.vsyn_cqt_num_frames(C.byref(_raw()), 0) == 0
    bt = synth_batch(fixture_like_spec(2), streams=3, packets_per_stream=12, pattern="mixed", seed=31)
    S = len(bt["segments"])
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    try:
        assert g.submit_host(bt["packets"], bt["segments"], bt["ys"], bt["residue"], bt["plane_stride"], flags=4)["rc"] == 0
        for spec, null_rates in [(_raw(**kw), False) for kw in BAD_SPECS] + [(_raw(), True)]:
            rates = np.full(S, 8000, np.uint32)
            seg_rows, rows, ref = np.full(S, 77, np.uint64), np.full((64, 24), 77.0, np.float32), np.full(S, 77, np.uint32)
            err, st = C.c_char_p(), Status(77, 77)
            rc = g.lib.vsyn_pcm_cqt_host(g.h, C.byref(spec), S, None if null_rates else rates.ctypes.data, 0, rows.ctypes.data, 64,
                                         seg_rows.ctypes.data, ref.ctypes.data, C.byref(st), C.byref(err))
            assert rc == 1 and err.value
            assert (seg_rows == 77).all() and (rows == 77).all() and (ref == 77).all() and (st.flags, st.first_bad_packet) == (77, 77)
        # the host form on the last submit's PCM equals the device form on the fetched PCM, natively and behind the resampler
        from parseoggvorbis_amd.binding import VSYN_PCM_F32
        spec = _spec(fmin=400.0, n_bins=9, bins_per_octave=4, hop_length=37)[0]
        f1, fr = g.pcm_fetch_host(VSYN_PCM_F32, S, bt["plane_stride"])
        rates = ([16000, 0, 8000] + [16000] * S)[:S]
        host = g.pcm_cqt_host(spec, rates)
        x = np.zeros((S, 2, int(fr.max()) + 4), np.float32)
        for gi in range(S):
            x[gi, :, :int(fr[gi])] = f1[gi, :int(fr[gi])].T
        dev = _run(synth, spec, x, [int(v) for v in fr], rates)
        assert host["rc"] == 0 and not host["refused"].any() and int(host["seg_rows"][1]) == 0 and int(host["seg_rows"].sum()) > 0
        assert np.array_equal(host["seg_rows"], np.diff(dev["off"]).astype(np.uint64))
        assert np.array_equal(_bits(host["rows"]), _bits(np.concatenate(dev["rows"])))
        low = g.pcm_cqt_host(spec, rates, 12000)
        assert int(low["seg_rows"][1]) == 0 and low["rows"].shape[0] == int(low["seg_rows"].sum()) > 0 and np.isfinite(low["rows"]).all()
    finally:
        g.close()
    # the accepted side of the caps: L_0 = 2^17 exactly (bpo = 1, Q = 1, N_0 = sr / fmin)
    cap = dict(fmin=65536.0 / (1 << 17), n_bins=1, bins_per_octave=1, filter_scale=3.0 / 5.0, hop_length=50000)
    assert m.lengths(m.spec(**cap), 65536)[1] == [1 << 17]
    # a tone at the bin's own 0.5 Hz under the noise, so that every chunk carries weight in the sum: a chunk lost or counted twice
    # moves the coefficient by about 1 / 128 of itself, a thousand bounds
    x = _signal(1, 70000, 65536, 77)
    x = (x + 0.4 * np.cos(2.0 * np.pi * 0.5 * np.arange(70000) / 65536.0 + 0.3)[None, :]).astype(np.float32)
    worst = _one(synth, cap, 65536, 70000, x=x)
    print("constant-Q at L_0 = 2^17: worst |d| / bound %.6f" % worst)
    assert worst < 1.0
