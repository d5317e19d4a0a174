"""Chroma and tonnetz rows on the GPU (include/vorbis_synth_hip.h, "chroma"): every value of every case against the float64 model
under the per-frame bound derived in tests/chroma_model.py; nothing is excluded, no factor is fitted. The inputs hold
no frame with 0 < N < 1e-30 (the model asserts it), so that the FLT_MIN rule cannot differ between model and device.

Measured on the MI355X, worst |d| / bound over the grid (every norm, both powers, the chroma arguments off their defaults):
FFT path chroma 0.058 (n_fft 16), 0.042 (64), 0.012 (2048), 0.011 (8192), tonnetz at most 0.007; direct path chroma 0.032 (n_fft 48),
0.011 (1102), tonnetz at most 0.003; one cosine per bin 0.033; end to end from Ogg bytes chroma at most 0.009 (DESIGN.md 6n has the
table). The S term of the bound, a worst case over n_fft roundings, dominates it, as in the linear spectra's tests."""
import ctypes as C

import numpy as np
import pytest

from tests import chroma_model as cm
from tests import spectral_lin_model as lm
from tests import spectral_model as sm
from tests import spectral_post_model as pm
from tests.test_gpu_spectral import _ogg
from tests.test_gpu_spectral_lin import mono_batch
from tests.test_gpu_spectral_post import _delta_bound

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
E2E_FILES = ["test.mono44khz", "test.stereo44khz", "synth_04"]
KINDS = ("chroma", "tonnetz")
NORMS = (np.inf, 1, 2, None)
# the chroma arguments off their defaults, one at a time and together
CHROMA_VARIANTS = [dict(n_chroma=36), dict(base_c=False), dict(octwidth=None), dict(tuning=0.37),
                   dict(n_chroma=36, base_c=False, octwidth=None, tuning=0.37, chroma_norm=2)]
# n_fft -> hop: four FFT-path sizes and two direct-path sizes
GRID_HOPS = {16: 5, 64: 16, 2048: 512, 8192: 2048, 48: 12, 1102: 441}


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


def run_chroma(g, spec, chroma, pcm, frames, rates, offset=0, plain_entry=False):
    """run_device of tests/test_gpu_spectral_lin.py through vsyn_spectral_chroma_device (chroma may be None: the defaults), or with
    plain_entry through vsyn_spectral_device itself: the list of each segment's rows; the rows buffer is NaN-filled and must stay so
    past the last row. (run_device sizes its rows by spec_dim(spec), which is vsyn_spectral_dim and 0 for these kinds.)"""
    import torch
    from parseoggvorbis_amd import spectral
    pcm = np.ascontiguousarray(pcm, np.float32)
    S, Cn, plane = pcm.shape
    dim = spectral.spec_dim(spec, chroma if chroma is not None else spectral.chroma_spec())
    assert dim > 0
    fmax = sm.num_frames(plane, spec.n_fft, spec.hop_length, bool(spec.options & spectral.OPT_CENTER))
    buf = torch.zeros(pcm.size + 8, dtype=torch.float32, device="cuda")
    buf[offset:offset + pcm.size] = torch.from_numpy(pcm.reshape(-1)).cuda()
    d_frames = torch.from_numpy(np.asarray(frames, np.int32)).cuda()
    d_rows = torch.full((S * fmax + 1, dim), float("nan"), dtype=torch.float32, device="cuda")
    d_off = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    args = (rates, buf.data_ptr() + 4 * offset, plane, Cn, d_frames.data_ptr(), d_rows.data_ptr(), d_off.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if plain_entry:
        assert chroma is None
        g.spectral_device(spec, *args)
    else:
        g.spectral_chroma_device(spec, chroma, *args)
    torch.cuda.synchronize()
    off, rows = d_off.cpu().numpy(), d_rows.cpu().numpy()
    assert off[0] == 0 and off[S] <= S * fmax
    assert np.isnan(rows[off[S]:]).all()  # nothing written past the rows
    return [rows[off[i]:off[i + 1]] for i in range(S)]


def specs(spec_mod, kind, ckw, **skw):
    """(spectral spec, chroma struct, the model's keywords) of one case."""
    spec = spec_mod.spectral_spec(kind, **skw)
    chroma = spec_mod.chroma_spec(**ckw)
    mkw = dict(ckw, win_length=skw.get("win_length"), center=skw.get("center", True), power=int(skw.get("power", 2)))
    return spec, chroma, mkw


def signals(T, n_fft):
    """The inputs of lm.signals at any length T >= 0 (seeded noise, an off-bin sine plus 1e-4 noise, DC), and a burst beside exact
    silence: frames are exactly silent or clearly not."""
    rng = np.random.default_rng(n_fft)
    t = np.arange(T, dtype=np.float64)
    noise = 0.3 * rng.standard_normal(T)
    sine = 0.7 * np.sin(2.0 * np.pi * (5.37 / n_fft) * t + 0.3) + 1e-4 * rng.standard_normal(T)
    dc = np.full(T, 0.25)
    burst = np.zeros(T)
    a, b = min(T // 3, T), min(T // 3 + max(n_fft // 2, 8), T)
    burst[a:b] = 0.9 * rng.standard_normal(b - a)
    return {k: v.astype(np.float32) for k, v in (("noise", noise), ("sine", sine), ("dc", dc), ("burst", burst))}


def length_for(F, n_fft, hop, center):
    """A signal length that gives exactly F frames."""
    if F == 0:
        return 0
    return max(1, hop * (F - 1)) if center else n_fft + hop * (F - 1)


@pytest.mark.parametrize("n_fft", [64, 48])
def test_one_bin_centred_cosine_per_bin(spec_mod, synth, n_fft):
    """hop = n_fft, no centring, chroma_norm=None: segment k0 holds cos(2 pi k0 t / n_fft), whose Hann-windowed power spectrum is
    (n/4)^2 at k0 and (n/8)^2 at k0 +- 1, so the row is that combination of three columns of W: any slip of k or c shows."""
    t = np.arange(2 * n_fft, dtype=np.float64)
    ks = list(range(1, n_fft // 2))
    pcm, frames = mono_batch([np.cos(2.0 * np.pi * k0 * t / n_fft).astype(np.float32) for k0 in ks])
    for sr in (22050, 8000):
        spec, chroma, mkw = specs(spec_mod, "chroma", dict(chroma_norm=None), n_fft=n_fft, hop_length=n_fft, center=False)
        rows = run_chroma(synth, spec, chroma, pcm, frames, [sr] * len(ks))
        W = cm.filterbank32(sr, n_fft).astype(np.float64)
        worst = 0.0
        for k0, r in zip(ks, rows):
            assert r.shape == (2, 12)
            worst = max(worst, cm.check(r, pcm[k0 - 1, 0], "chroma", sr, n_fft, n_fft, what=("cosine", n_fft, k0), **mkw))
            want = (n_fft / 4.0) ** 2 * W[:, k0] + (n_fft / 8.0) ** 2 * (W[:, k0 - 1] + (W[:, k0 + 1] if k0 + 1 <= n_fft // 2 else 0.0))
            if k0 + 1 == n_fft // 2:  # the neighbour at Nyquist gets both sidebands: (n/4)^2 there
                want = want + ((n_fft / 4.0) ** 2 - (n_fft / 8.0) ** 2) * W[:, k0 + 1]
            if k0 == 1:  # and so does DC
                want = want + ((n_fft / 4.0) ** 2 - (n_fft / 8.0) ** 2) * W[:, 0]
            assert np.allclose(r[0], want, rtol=1e-4, atol=1e-4 * want.max()), (n_fft, sr, k0)
        print("cosines n_fft %d sr %d: worst |d| / bound %.3f" % (n_fft, sr, worst))


@pytest.mark.parametrize("center", [False, True], ids=["nc", "c"])
@pytest.mark.parametrize("n_fft", sorted(GRID_HOPS))
def test_the_grid_against_the_model(spec_mod, synth, n_fft, center):
    """Noise, an off-bin sine, DC and a burst beside exact silence at tile - 1, tile + 1 and 2 tile frames (the tile read from the
    library), rates 22050 and 44100 alternating in one batch (the per-rate tables are picked per segment); both kinds at every norm
    and both powers, then the chroma arguments off their defaults. win_length < n_fft without centring."""
    hop = GRID_HOPS[n_fft]
    win = n_fft if center else 3 * n_fft // 4 + 1
    probe = spec_mod.spectral_spec("chroma", n_fft=n_fft, hop_length=hop, win_length=win, center=center)
    tile = synth.lib.vsyn_spectral_chroma_tile(C.byref(probe))
    assert tile >= 1 and tile == (synth.lib.vsyn_spectral_lin_tile(C.byref(spec_mod.spectral_spec("stft", n_fft=n_fft, hop_length=hop)))
                                  if lm.is_pow2(n_fft) else tile)
    sigs, counts = [], []
    for F in (tile - 1, tile + 1, 2 * tile):
        T = length_for(F, n_fft, hop, center)
        assert sm.num_frames(T, n_fft, hop, center) == F
        s = signals(T, n_fft)
        sigs += [s[k] for k in sorted(s)]
        counts += [F] * len(s)
    pcm, frames = mono_batch(sigs)
    rates = [22050 if i % 2 == 0 else 44100 for i in range(len(sigs))]
    cases = [(kind, dict(chroma_norm=norm), power) for kind in KINDS for norm in NORMS for power in (2, 1)]
    cases += [(kind, ckw, 2) for kind in KINDS for ckw in CHROMA_VARIANTS]
    worst = {}
    for kind, ckw, power in cases:
        spec, chroma, mkw = specs(spec_mod, kind, ckw, n_fft=n_fft, hop_length=hop, win_length=win, center=center, power=power)
        rows = run_chroma(synth, spec, chroma, pcm, frames, rates)
        assert [r.shape[0] for r in rows] == counts
        for i, (y, r) in enumerate(zip(sigs, rows)):
            e = cm.check(r, y, kind, rates[i], n_fft, hop, what=(n_fft, center, i, kind, ckw, power), **mkw)
            worst[kind] = max(worst.get(kind, 0.0), e)
    print("n_fft %d %s tile %d: worst |d| / bound %s" % (n_fft, "centred" if center else "not centred", tile,
                                                         " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("n_fft", [64, 48])
def test_frame_edges_and_a_skipped_segment(spec_mod, synth, n_fft):
    """T = 0, 1, n_fft - 1, n_fft; a segment of rate 0 between two live ones gets no rows; nothing is written past the last row
    (run_chroma asserts that the NaN fill stays)."""
    rng = np.random.default_rng(n_fft)
    hop = n_fft // 4
    lens = [0, 1, n_fft - 1, n_fft, 5 * n_fft, 3 * n_fft]
    rates = [22050, 22050, 44100, 22050, 0, 44100]
    sigs = [(0.3 * rng.standard_normal(t)).astype(np.float32) for t in lens]
    pcm, frames = mono_batch(sigs)
    for center in (False, True):
        want = [sm.num_frames(t, n_fft, hop, center) if r else 0 for t, r in zip(lens, rates)]
        assert want[0] == 0 and want[4] == 0 and want[3] >= 1 and want[5] > 1 and (center or want[2] == 0)
        for kind in KINDS:
            spec, chroma, mkw = specs(spec_mod, kind, {}, n_fft=n_fft, hop_length=hop, center=center)
            rows = run_chroma(synth, spec, chroma, pcm, frames, rates)
            assert [r.shape[0] for r in rows] == want
            for y, r, sr in zip(sigs, rows, rates):
                if sr:
                    cm.check(r, y, kind, sr, n_fft, hop, what=("edges", n_fft, center, len(y), kind), **mkw)


@pytest.mark.parametrize("n_fft", [64, 48])
def test_silence_gives_zero_rows_under_every_norm(spec_mod, synth, n_fft):
    pcm = np.zeros((2, 2, 10 * n_fft), np.float32)
    for kind in KINDS:
        for norm in NORMS:
            spec, chroma, _ = specs(spec_mod, kind, dict(chroma_norm=norm), n_fft=n_fft, hop_length=n_fft // 4)
            for r in run_chroma(synth, spec, chroma, pcm, [10 * n_fft, 3 * n_fft], [22050, 44100]):
                assert r.shape[0] > 0 and np.array_equal(r, np.zeros_like(r)), (kind, norm)


@pytest.mark.parametrize("n_fft", [64, 48])
def test_a_non_finite_sample_makes_exactly_its_frames_nan(spec_mod, synth, n_fft):
    """One NaN sample and one Inf sample: the frames that hold them are all NaN under both kinds and every norm, their neighbours
    meet the bound (cm.check asserts both, from the model's own non-finite rule)."""
    rng = np.random.default_rng(5)
    hop, T = n_fft // 4, 24 * n_fft // 4
    a = (0.3 * rng.standard_normal(T)).astype(np.float32)
    b = a.copy()
    a[7 * hop + 3] = np.nan
    b[11 * hop] = np.inf
    pcm, frames = mono_batch([a, b])
    for kind in KINDS:
        for norm in NORMS:
            spec, chroma, mkw = specs(spec_mod, kind, dict(chroma_norm=norm), n_fft=n_fft, hop_length=hop)
            rows = run_chroma(synth, spec, chroma, pcm, frames, [22050, 22050])
            for y, r in zip((a, b), rows):
                nan_rows = np.isnan(r).all(axis=1)
                assert 4 <= int(nan_rows.sum()) <= 5 and not nan_rows[0] and not nan_rows[-1]
                cm.check(r, y, kind, 22050, n_fft, hop, what=("non-finite", n_fft, kind, norm), **mkw)


@pytest.mark.parametrize("n_fft,hop", [(64, 16), (1024, 256), (1102, 441)])
def test_same_bits(spec_mod, synth, n_fft, hop):
    """A segment alone, as slot 0 and as slot 2 of a batch, at plane offsets 0 and 3 floats, and with its frames shifted by a whole
    hop within the tile: the same bits."""
    rng = np.random.default_rng(3)
    T = 5000
    y = (0.3 * rng.standard_normal(T)).astype(np.float32)
    others = (0.9 * rng.standard_normal((4, 1, T))).astype(np.float32)
    for kind, ckw in (("chroma", {}), ("tonnetz", dict(chroma_norm=2, n_chroma=36))):
        spec, chroma, _ = specs(spec_mod, kind, ckw, n_fft=n_fft, hop_length=hop, center=False)
        alone = run_chroma(synth, spec, chroma, y[None, None, :], [T], [44100])[0]
        assert alone.shape[0] > 2 and np.isfinite(alone).all()
        for slot in (0, 2):
            batch = others.copy()
            batch[slot, 0] = y
            fr = [4000, 4000, 4000, 3000]
            fr[slot] = T
            assert np.array_equal(run_chroma(synth, spec, chroma, batch, fr, [44100, 22050, 44100, 22050])[slot], alone), slot
        assert np.array_equal(run_chroma(synth, spec, chroma, y[None, None, :], [T], [44100], offset=3)[0], alone)
        shifted = run_chroma(synth, spec, chroma, y[None, None, hop:], [T - hop], [44100])[0]
        assert np.array_equal(shifted, alone[1:1 + shifted.shape[0]]) and shifted.shape[0] == alone.shape[0] - 1


@pytest.mark.parametrize("n_fft,hop", [(512, 128), (1102, 441)])
def test_default_routes_agree(spec_mod, synth, n_fft, hop):
    """vsyn_spectral_device with kind 8 / 9 equals vsyn_spectral_chroma_device with NULL and with an explicit default struct."""
    rng = np.random.default_rng(9)
    pcm = (0.3 * rng.standard_normal((3, 2, 4000))).astype(np.float32)
    frames, rates = [4000, 2500, 3999], [44100, 22050, 8000]
    for kind in KINDS:
        spec = spec_mod.spectral_spec(kind, n_fft=n_fft, hop_length=hop)
        a = run_chroma(synth, spec, None, pcm, frames, rates, plain_entry=True)
        b = run_chroma(synth, spec, None, pcm, frames, rates)
        c = run_chroma(synth, spec, spec_mod.chroma_spec(), pcm, frames, rates)
        for x, y, z, fr, sr, p in zip(a, b, c, frames, rates, pcm):
            assert x.shape[0] > 0 and np.array_equal(x, y) and np.array_equal(x, z)
            cm.check(x, p[:, :fr], kind, sr, n_fft, hop, what=("default", kind, sr))  # (two channels: the downmix term of the bound)


# ---- end to end through get_spectral_batch ----

E2E = [("chroma", dict(n_fft=2048, hop_length=512)), ("tonnetz", dict(n_fft=1102, hop_length=441)),
       ("chroma", dict(n_fft=1024, hop_length=256, n_chroma=24, chroma_norm=2, tuning=-0.2, power=1))]
CHROMA_KEYS = ("n_chroma", "tuning", "chroma_norm", "ctroct", "octwidth", "base_c")


def _model_kw(kw):
    return {k: v for k, v in kw.items() if k in CHROMA_KEYS + ("win_length", "center", "power")}


@pytest.mark.parametrize("stage", [{}, dict(sr=22050), dict(trim_db=30), dict(preemphasis=0.97)], ids=["plain", "sr", "trim", "preemph"])
def test_end_to_end_against_the_model(spec_mod, stage):
    """The rows equal the model on the mono signal that get_pcm_batch(mono=True, same stage arguments) returns, within the bound."""
    from parseoggvorbis_amd import pcm as pcm_mod
    datas = [_ogg(n) for n in E2E_FILES]
    sig = pcm_mod.get_pcm_batch(datas, mono=True, **stage)
    for kind, kw in E2E:
        res = spec_mod.get_spectral_batch(datas, kind=kind, **kw, **stage)
        for name, (y, rate), got in zip(E2E_FILES, sig, res):
            assert y.ndim == 1 and y.dtype == np.float32
            assert got.shape[0] == sm.num_frames(len(y), kw["n_fft"], kw["hop_length"]) > 0 and got.shape[1] == (6 if kind == "tonnetz" else kw.get("n_chroma", 12))
            e = cm.check(got, y, kind, rate, kw["n_fft"], kw["hop_length"], what=(name, kind, stage), **_model_kw(kw))
            print("%s %s %s: worst |d| / bound %.3f" % (name, kind, stage, e))


def test_end_to_end_with_delta_and_normalisation(spec_mod):
    """delta=1, normalize="mean_var" behind both kinds, compared as tests/test_gpu_spectral_post.py compares the mel kinds: the rows'
    own bound pushed through the delta filter plus the filter's rounding, then (2 + |Z|) eps' / max(sigma, std_floor) + u |Z|."""
    from parseoggvorbis_amd import pcm as pcm_mod
    datas = [_ogg(n) for n in E2E_FILES]
    sig = pcm_mod.get_pcm_batch(datas, mono=True)
    width, floor = 3, 1e-5  # (synth_04 is a fraction of a second long: a short hop and the narrowest delta window)
    for kind, kw in (("chroma", dict(n_fft=256, hop_length=64)), ("tonnetz", dict(n_fft=400, hop_length=100, n_chroma=24))):
        plain = spec_mod.get_spectral_batch(datas, kind=kind, **kw)
        res = spec_mod.get_spectral_batch(datas, kind=kind, delta=1, delta_width=width, normalize="mean_var", std_floor=floor, **kw)
        only_delta = spec_mod.get_spectral_batch(datas, kind=kind, delta=1, delta_width=width, **kw)
        for name, (y, rate), got, p, od in zip(E2E_FILES, sig, res, plain, only_delta):
            base, tol = cm.rows(y, kind, rate, kw["n_fft"], kw["hop_length"], **_model_kw(kw))
            D = base.shape[1]
            assert got.shape == od.shape == (base.shape[0], 2 * D) and base.shape[0] >= width and np.array_equal(od[:, :D], p)
            yd = pm.with_deltas(base, 1, width)
            epsb = np.concatenate([tol, pm.delta(tol, width, 1, coefs=np.abs(pm.delta_coefs(width, 1))) + _delta_bound(base, width, 1)], axis=1)
            d = np.abs(od.astype(np.float64) - yd)
            assert (d <= epsb).all(), (name, kind, "delta", float((d / np.maximum(epsb, 1e-300)).max()))
            want = pm.post(base, 1, width, "mean_var", floor)
            sigma = pm.stats(yd)[1]
            tz = (2.0 + np.abs(want)) * epsb.max(axis=0) / np.maximum(sigma, floor) + U * np.abs(want)
            d = np.abs(got.astype(np.float64) - want)
            assert (d <= tz).all(), (name, kind, "mean_var", float((d / tz).max()))


def test_a_damaged_file_fails_alone(spec_mod):
    names = ["test.stereo44khz", "synth_04", "test.mono44khz"] * 2
    blobs = [_ogg(n) for n in names]
    bad = bytearray(blobs[4])
    bad[len(bad) // 2] ^= 0x55  # a page CRC
    blobs[4] = bytes(bad)
    kw = dict(kind="chroma", n_fft=1024, hop_length=256)
    res = spec_mod.get_spectral_batch(blobs, errors="return", files_per_submit=4, **kw)
    single = {n: spec_mod.get_spectral_from_raw_bytes(_ogg(n), **kw) for n in set(names)}
    for i, (n, r) in enumerate(zip(names, res)):
        if i == 4:
            assert isinstance(r, spec_mod.SpectralError) and "file 4" in str(r)
            continue
        assert isinstance(r, np.ndarray) and r.dtype == np.float32 and r.shape[1] == 12, (i, r)
        assert np.array_equal(r, single[n]), i


def test_existing_kinds_through_the_chroma_entry_are_the_existing_entries(spec_mod):
    """ogg_vorbis_spectral_corpus_chroma with chroma = NULL and a kind <= 7 (every other stage's spec NULL, then a trim and the post
    stage on) gives the bits of the entries get_spectral_batch takes for those kinds; with kind 8 and NULL, the default arguments'."""
    from parseoggvorbis_amd import _corpus, pcm as pcm_mod
    from parseoggvorbis_amd.binding import LOUDNESS_RECORD_DTYPE
    datas = [_ogg(n) for n in E2E_FILES]
    lib = spec_mod._load()
    n = len(datas)

    def through_chroma_entry(spec, dim, post=None, gate=None):
        counts = np.zeros(n, np.uint64)
        ib = _corpus.IntervalBuffers(lib, n)
        joined, bounds, records = np.zeros(n, np.uint64), np.zeros((n, 2), np.uint64), np.zeros(n, LOUDNESS_RECORD_DTYPE)
        try:
            return _corpus.run(lib, lib.ogg_vorbis_spectral_corpus_chroma, datas,
                               (0, 0, 64, 0, C.byref(spec), None, 0, None, None if post is None else C.byref(post), None,
                                None if gate is None else C.byref(gate), 0, None), (counts, bounds, joined, ib.ptrs, ib.counts, records),
                               lambda i, p: _corpus.copy_into(np.zeros((int(counts[i]), dim), np.float32), p), spec_mod.SpectralError, "return",
                               "spectral")
        finally:
            ib.free()

    def same(got, want, what):
        arrays = 0
        for a, b in zip(got, want):
            if isinstance(b, Exception):  # (a file trimmed below the delta window fails alone, by the same words)
                assert isinstance(a, Exception) and str(a) == str(b), what
            else:
                assert a.shape[0] > 0 and np.array_equal(a, b), what
                arrays += 1
        assert arrays >= 2, what

    for kind, kw in (("log_mel", dict(n_fft=400, hop_length=100, n_mels=40)), ("mfcc", dict(n_fft=512, hop_length=64)),
                     ("lin_power", dict(n_fft=512, hop_length=128)), ("chroma", dict(n_fft=512, hop_length=64))):
        spec = spec_mod.spectral_spec(kind, **kw)
        dim = spec_mod.spec_dim(spec, spec_mod.chroma_spec())
        same(through_chroma_entry(spec, dim), spec_mod.get_spectral_batch(datas, kind=kind, errors="return", **kw), kind)
        if kind == "lin_power":
            continue
        post, dout, _ = spec_mod.post_spec(dim, delta=1, delta_width=3)
        trim = pcm_mod.trim_spec(30, 2048, 512, None, spec_mod.SpectralError)
        want = spec_mod.get_spectral_batch(datas, kind=kind, delta=1, delta_width=3, trim_db=30, errors="return", **kw)
        same(through_chroma_entry(spec, dout, post, trim), want, (kind, "trim + delta"))
