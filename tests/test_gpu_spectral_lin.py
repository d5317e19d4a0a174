"""Linear spectra on the GPU (include/vorbis_synth_hip.h, "linear spectra"): every value of every case against the float64 model
under the derived per-frame bound of tests/spectral_lin_model.py (K = 4 (log2 n_fft + 2) on the FFT path, win_length + 3 on the
direct path; the bounds of lin_power and lin_db follow from it). Multi-channel inputs use the general downmix term of the bound
((C + 1) u mean_c |x_c| per sample, weighted by the window), not quantised inputs. No value is excluded anywhere.

Measured on the MI355X (worst |d| / bound over the grid; DESIGN.md 6k has the table per kind and n_fft): stft 0.024 ... 0.159,
lin_power 0.016 ... 0.115; on the FFT path stft is at most 0.122 (n_fft 64), i.e. 3.9 u A_f. lin_db is checked as an interval and
reaches its end only where that end is the clamp (bins that are zero to rounding)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import spectral_lin_model as lm
from tests import spectral_model as sm
from tests.test_gpu_spectral import GOLDEN, _decode_pcm, _ogg, _rate, _rehead

pytestmark = pytest.mark.gpu

E2E_FILES = ["test.mono44khz", "test.stereo44khz", "synth_04"]
VARIANTS = [("stft", {}), ("lin_power", dict(power=2)), ("lin_power", dict(power=1)), ("lin_db", dict(power=2)), ("lin_db", dict(power=1))]


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


@pytest.fixture(scope="module")
def product_pcm(spec_mod):
    return dict(zip(E2E_FILES, _decode_pcm([_ogg(n) for n in E2E_FILES])))


def run_device(g, spec, pcm, frames, rates, offset=0):
    """vsyn_spectral_device on pcm [S][C][plane] float32 placed `offset` floats into a device buffer: the list of each segment's
    rows (float32 [F_g][dim]). Rows past the last segment's must stay untouched."""
    import torch
    from parseoggvorbis_amd import spectral
    pcm = np.ascontiguousarray(pcm, np.float32)
    S, Cn, plane = pcm.shape
    dim = spectral.spec_dim(spec)
    fmax = sm.num_frames(plane, spec.n_fft, spec.hop_length, bool(spec.options & spectral.OPT_CENTER))
    buf = torch.zeros(pcm.size + 8, dtype=torch.float32, device="cuda")
    buf[offset:offset + pcm.size] = torch.from_numpy(pcm.reshape(-1)).cuda()
    d_frames = torch.from_numpy(np.asarray(frames, np.int32)).cuda()
    d_rows = torch.full((S * fmax + 1, dim), float("nan"), dtype=torch.float32, device="cuda")
    d_off = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    g.spectral_device(spec, rates, buf.data_ptr() + 4 * offset, plane, Cn, d_frames.data_ptr(), d_rows.data_ptr(), d_off.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    off, rows = d_off.cpu().numpy(), d_rows.cpu().numpy()
    assert off[0] == 0 and off[S] <= S * fmax
    assert np.isnan(rows[off[S]:]).all()  # nothing written past the rows
    return [rows[off[i]:off[i + 1]] for i in range(S)]


def mono_batch(signals):
    """Mono signals of different lengths as one batch: (pcm [S][1][plane], frames)."""
    plane = max(max(len(y) for y in signals), 1)
    pcm = np.zeros((len(signals), 1, plane), np.float32)
    for i, y in enumerate(signals):
        pcm[i, 0, :len(y)] = y
    return pcm, [len(y) for y in signals]


@pytest.mark.parametrize("n_fft", [16, 64])
def test_unit_impulse_at_every_position(spec_mod, synth, n_fft):
    """hop 1 over one impulse, no centring, win_length = n_fft: frame f holds the impulse at p = 2 n - 1 - f, every p of a frame,
    and X_k = w_p exp(-2 pi i p k / n) differs for every (p, k): any slip of an index in a pass or in the untangling shows."""
    y = np.zeros(3 * n_fft, np.float32)
    y[2 * n_fft - 1] = 1.0
    for kind, kw in VARIANTS:
        spec = spec_mod.spectral_spec(kind, n_fft=n_fft, hop_length=1, center=False, **kw)
        rows = run_device(synth, spec, y[None, None, :], [len(y)], [44100])[0]
        assert rows.shape[0] == 2 * n_fft + 1
        lm.check(rows, y, kind, n_fft, 1, None, False, what=("impulse", n_fft, kind, kw), **kw)
        if kind == "stft":  # and the rows are not trivially zero: row f has |X_k| = w_p for every k
            p = 2 * n_fft - 1 - np.arange(n_fft, 2 * n_fft)
            mag = np.abs(rows.view(np.complex64)[n_fft:2 * n_fft])
            assert np.allclose(mag, sm.window(n_fft)[p][:, None], atol=1e-5)


@pytest.mark.parametrize("entry", lm.GRID, ids=lambda e: "n%d_h%d_w%d_%s" % (e[0], e[1], e[2], "c" if e[3] else "nc"))
def test_the_grid_against_the_model(spec_mod, synth, entry):
    """Noise, an off-bin sine plus 1e-4 noise, DC, and a loud burst beside a near-silent stretch, one segment each in one batch;
    every kind (lin_power and lin_db at both powers) at every framing of the grid."""
    n, hop, win, center, T = entry
    sig = lm.signals(T, n)
    names = sorted(sig)
    pcm, frames = mono_batch([sig[k] for k in names])
    worst = {}
    for kind, kw in VARIANTS:
        spec = spec_mod.spectral_spec(kind, n_fft=n, hop_length=hop, win_length=win, center=center, **kw)
        rows = run_device(synth, spec, pcm, frames, [44100] * len(names))
        for name, r in zip(names, rows):
            assert r.shape[0] == sm.num_frames(T, n, hop, center) > 0
            e = lm.check(r, sig[name], kind, n, hop, win, center, what=(entry, name, kind, kw), **kw)
            key = kind + ("" if kind == "stft" else "/%d" % kw["power"])
            worst[key] = max(worst.get(key, 0.0), e)
    print("n_fft %d hop %d win %d: worst |d| / bound %s" % (n, hop, win, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("n_fft,hop", [(64, 16), (1102, 441), (2048, 512), (8192, 2048)])
def test_frame_count_edges(spec_mod, synth, n_fft, hop):
    """T = 0 and 1, T = n_fft - 1 (no frame without centring), T = n_fft exactly, and frame counts of tile + 1 and 2 tile, the tile
    read from the library."""
    rng = np.random.default_rng(n_fft)
    for center in (False, True):
        spec = spec_mod.spectral_spec("stft", n_fft=n_fft, hop_length=hop, center=center)
        tile = synth.lib.vsyn_spectral_lin_tile(C.byref(spec))
        assert tile >= 1
        p = 2 * (n_fft // 2) if center else 0
        lens = [0, 1, n_fft - 1, n_fft, n_fft - p + hop * tile, n_fft - p + hop * (2 * tile - 1) + hop - 1]
        lens = [max(t, 0) for t in lens]
        sigs = [(0.3 * rng.standard_normal(t)).astype(np.float32) for t in lens]
        pcm, frames = mono_batch(sigs)
        want = [sm.num_frames(t, n_fft, hop, center) for t in lens]
        assert want[0] == 0 and (center or want[2] == 0) and want[4] == tile + 1 and want[5] == 2 * tile
        for kind in ("stft", "lin_db"):
            spec = spec_mod.spectral_spec(kind, n_fft=n_fft, hop_length=hop, center=center)
            rows = run_device(synth, spec, pcm, frames, [8000] * len(lens))
            assert [r.shape[0] for r in rows] == want
            for y, r in zip(sigs, rows):
                lm.check(r, y, kind, n_fft, hop, None, center, what=("edges", n_fft, center, len(y), kind))


@pytest.mark.parametrize("n_fft,hop", [(512, 160), (1102, 441)])
def test_channels_and_batch_layout(spec_mod, synth, n_fft, hop):
    """C = 1, 2, 3; four segments with one of rate 0 and one empty; a plane_stride that is no multiple of 4."""
    rng = np.random.default_rng(7)
    plane = 3001
    for Cn in (1, 2, 3):
        pcm = (0.25 * rng.standard_normal((4, Cn, plane))).astype(np.float32)
        frames, rates = [3001, 2500, 0, 1777], [44100, 0, 16000, 8000]
        for kind, kw in VARIANTS[:2] + VARIANTS[3:4]:
            spec = spec_mod.spectral_spec(kind, n_fft=n_fft, hop_length=hop, **kw)
            rows = run_device(synth, spec, pcm, frames, rates)
            assert rows[1].shape[0] == 0 and rows[2].shape[0] == 0
            for gi in (0, 3):
                assert rows[gi].shape[0] == sm.num_frames(frames[gi], n_fft, hop)
                lm.check(rows[gi], pcm[gi, :, :frames[gi]], kind, n_fft, hop, what=("layout", Cn, gi, kind), **kw)


@pytest.mark.parametrize("n_fft,hop", [(64, 16), (1024, 256), (1102, 441)])
def test_bit_identity(spec_mod, synth, n_fft, hop):
    """The same segment alone, in slot 2 of a batch, at a plane offset of 1, 2 and 3 floats, and one frame further along its tile
    (the signal shifted by one hop): the same bits."""
    rng = np.random.default_rng(3)
    T = 5000
    y = (0.3 * rng.standard_normal(T)).astype(np.float32)
    others = (0.9 * rng.standard_normal((4, 1, T))).astype(np.float32)
    for kind in ("stft", "lin_db"):
        spec = spec_mod.spectral_spec(kind, n_fft=n_fft, hop_length=hop, center=False, top_db=None)
        alone = run_device(synth, spec, y[None, None, :], [T], [44100])[0]
        assert alone.shape[0] > 2 and np.isfinite(alone).all()
        batch = others.copy()
        batch[2, 0] = y
        assert np.array_equal(run_device(synth, spec, batch, [T, 4000, T, 3000], [44100] * 4)[2], alone)
        for off in (1, 2, 3):
            assert np.array_equal(run_device(synth, spec, y[None, None, :], [T], [44100], offset=off)[0], alone), off
        shifted = run_device(synth, spec, y[None, None, hop:], [T - hop], [44100])[0]
        assert np.array_equal(shifted, alone[1:1 + shifted.shape[0]]) and shifted.shape[0] == alone.shape[0] - 1


@pytest.mark.parametrize("top_db", [None, 80.0, 40.0])
def test_lin_db_clamp(spec_mod, synth, top_db):
    """The clamp is the model's clamp on the model's maximum, within the image bound; the burst signal spans far more than 80 dB."""
    for n, hop in ((512, 128), (1102, 441)):
        y = lm.signals(6000, n)["burst"]
        spec = spec_mod.spectral_spec("lin_db", n_fft=n, hop_length=hop, top_db=top_db)
        r = run_device(synth, spec, y[None, None, :], [len(y)], [44100])[0]
        lm.check(r, y, "lin_db", n, hop, top_db=top_db, what=("clamp", n, top_db))
        span = float(r.max() - r.min())
        if top_db:
            assert span == pytest.approx(top_db, abs=1e-4)
        else:
            assert span > 100.0


def test_a_linear_kind_leaves_the_pcm_and_the_next_submit_alone(spec_mod):
    """vsyn_pcm_spectral_host of a linear kind between two submits: vsyn_pcm_fetch_host and the next submit are bit-identical to a
    handle that made no spectral call; and the post stage with a linear kind is refused with the outputs untouched."""
    from parseoggvorbis_amd.binding import Status, Synth, VSYN_ERR_INVALID, VSYN_PCM_F32
    from tests.workloads import fixture_like_spec, synth_batch
    spec = fixture_like_spec(2)
    b1 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=11)
    b2 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=12)
    S = len(b1["segments"])
    outs = []
    for with_spectral in (False, True):
        g = Synth(spec, device=0, max_streams=4)
        r1 = g.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"], flags=4)  # KEEP_PCM
        assert r1["rc"] == 0
        f1, fr1 = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        if with_spectral:
            for kind, kw in (("stft", dict(n_fft=512, hop_length=128)), ("lin_db", dict(n_fft=400, hop_length=160)),
                             ("lin_power", dict(n_fft=2048, hop_length=512))):
                s = spec_mod.spectral_spec(kind, **kw)
                r = g.pcm_spectral_host(s, [44100] * S)
                assert r["rc"] == 0 and r["rows"].shape == (int(r["seg_rows"].sum()), spec_mod.spec_dim(s)) and r["rows"].shape[0] > 0
                o = 0
                for gi in range(S):
                    nr = int(r["seg_rows"][gi])
                    lm.check(r["rows"][o:o + nr], f1[gi, :fr1[gi]].T, kind, kw["n_fft"], kw["hop_length"], what=("host", gi, kind))
                    o += nr
            # refusal: a post spec with the stage on and a linear kind
            s = spec_mod.spectral_spec("lin_power", n_fft=512, hop_length=128)
            post, _, _ = spec_mod.post_spec(257, delta=1)
            rows = np.full((64, 514), 7.0, np.float32)
            seg_rows = np.full(S, 12345, np.uint64)
            rates = np.full(S, 44100, np.uint32)
            st, err = Status(), C.c_char_p()
            rc = g.lib.vsyn_pcm_spectral_post_host(g.h, C.byref(s), C.byref(post), S, rates.ctypes.data, 0, rows.ctypes.data, 64,
                                                   seg_rows.ctypes.data, C.byref(st), C.byref(err))
            assert rc == VSYN_ERR_INVALID and b"linear" in err.value
            assert (rows == 7.0).all() and (seg_rows == 12345).all()
        f1b, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        assert np.array_equal(f1, f1b)
        r2 = g.submit_host(b2["packets"], b2["segments"], b2["ys"], b2["residue"], b2["plane_stride"])
        assert r2["rc"] == 0
        outs.append((f1, r2["pcm"], r2["emit_len"]))
        g.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])


# ---- end to end through get_spectral_batch ----

E2E = [("lin_power", dict(n_fft=1024, hop_length=256)), ("stft", dict(n_fft=1102, hop_length=441))]


def test_end_to_end_against_the_model_on_the_products_pcm(spec_mod, product_pcm):
    datas = [_ogg(n) for n in E2E_FILES]
    for kind, kw in E2E:
        res = spec_mod.get_spectral_batch(datas, kind=kind, **kw)
        mel = spec_mod.get_spectral_batch(datas, kind="log_mel", n_mels=8, **kw)
        for name, got, m in zip(E2E_FILES, res, mel):
            x = product_pcm[name]
            nb = kw["n_fft"] // 2 + 1
            assert got.shape == (sm.num_frames(x.shape[1], kw["n_fft"], kw["hop_length"]), nb) and got.shape[0] == m.shape[0] > 0
            assert got.dtype == (np.complex64 if kind == "stft" else np.float32)
            e = lm.check(got, x, kind, kw["n_fft"], kw["hop_length"], what=(name, kind))
            print("%s %s: worst |d| / bound %.3f" % (name, kind, e))


def test_end_to_end_against_the_reference_pcm(spec_mod, product_pcm):
    """The model on the reference decoder's PCM (tests/golden/<name>.npz); the gate is widened by sum_j w_j |dy_j| from the
    measured difference of the two mono signals."""
    for name in E2E_FILES:
        ref = np.load(os.path.join(GOLDEN, name + ".npz"))["pcm"].astype(np.float64)
        mine = product_pcm[name].astype(np.float64)
        assert ref.shape == mine.shape
        assert float(np.abs(ref - mine).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max()))  # the PCM gate of the synthesis tests
        dy = np.abs(ref.mean(axis=0) - mine.mean(axis=0))
        for kind, kw in E2E:
            got = spec_mod.get_spectral_from_raw_bytes(_ogg(name), kind=kind, **kw)
            lm.check(got, ref, kind, kw["n_fft"], kw["hop_length"], extra=dy, what=(name, kind, "reference"))


@pytest.mark.parametrize("stage", [dict(sr=16000), dict(preemphasis=0.97, peak_normalize=True), dict(trim_db=40), dict(split_db=40)])
def test_composition_with_the_pcm_stages(spec_mod, stage):
    """The rows equal the model on the signal that get_pcm_batch(mono=True, same arguments) returns, within the bound, and the
    trim / split indices equal those of the PCM call."""
    from parseoggvorbis_amd import pcm as pcm_mod
    datas = [_ogg(n) for n in E2E_FILES]
    ti, si, ti2, si2 = [], [], [], []
    sig = pcm_mod.get_pcm_batch(datas, mono=True, trim_index=ti, split_index=si, **stage)
    for kind, kw in E2E:
        res = spec_mod.get_spectral_batch(datas, kind=kind, trim_index=ti2, split_index=si2, **kw, **stage)
        for name, (y, _), got in zip(E2E_FILES, sig, res):
            assert y.ndim == 1 and y.dtype == np.float32
            lm.check(got, y, kind, kw["n_fft"], kw["hop_length"], what=(name, kind, stage))
        assert ti2 == ti
        assert len(si2) == len(si) and all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(si, si2))


def test_rows_do_not_depend_on_the_rate(spec_mod):
    """A batch of mixed rates (the same stream re-headed): the linear rows are the same bits at every rate, fmax or not."""
    data = _ogg("test.stereo44khz")
    blobs = [data, _rehead(data, 16000), _rehead(data, 8000), data]
    assert _rate(blobs[1]) == 16000
    for kind, kw in E2E:
        res = spec_mod.get_spectral_batch(blobs, kind=kind, **kw)
        for r in res[1:]:
            assert np.array_equal(r, res[0])
    low = spec_mod.get_spectral_batch(blobs, kind="log_mel", n_fft=1024, hop_length=256, errors="return", fmax=11025.0)
    assert isinstance(low[1], spec_mod.SpectralError)  # the mel kinds do depend on it


def test_a_damaged_file_fails_alone(spec_mod):
    names = ["test.stereo44khz", "synth_04", "test.mono44khz"] * 2
    blobs = [_ogg(n) for n in names]
    bad = bytearray(blobs[4])
    bad[len(bad) // 2] ^= 0x55  # a page CRC
    blobs[4] = bytes(bad)
    kw = dict(kind="stft", n_fft=1024, hop_length=256)
    res = spec_mod.get_spectral_batch(blobs, errors="return", files_per_submit=4, **kw)
    single = {n: spec_mod.get_spectral_from_raw_bytes(_ogg(n), **kw) for n in set(names)}
    for i, (n, r) in enumerate(zip(names, res)):
        if i == 4:
            assert isinstance(r, spec_mod.SpectralError) and "file 4" in str(r)
            continue
        assert isinstance(r, np.ndarray) and r.dtype == np.complex64, (i, r)
        assert np.array_equal(r, single[n]), i
