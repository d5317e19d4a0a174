"""Resampling on the GPU (vsyn_resample_device, vsyn_pcm_resample_host, vsyn_pcm_resample_spectral_host, ogg_vorbis_pcm_corpus,
parseoggvorbis_amd/pcm.py, spectral.get_spectral_batch(sr=...)) against the float64 model of tests/resample_model.py.

Gates: the taps are float32 and each output is one float32 FMA chain of K = ceil(N / up) terms (21 to 56 for the usual pairs), so
an output is good to a few float32 ulps of max|x|: |d| <= 2e-6 * max(1, max|x|). Up == down is the input, bit for bit. Corpus
PCM against the model over the reference decoder's PCM: 1e-5 * max(1, max|x|), the project's PCM gate (the synthetic fixtures
reach |x| = 2307). int16: 1 LSB."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from tests import resample_model as rm
from tests import spectral_model as sm
from tests.workloads import ogg_crc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HOST = os.path.join(ROOT, "parseoggvorbis_amd", "host")
FILES = ["test.stereo44khz", "test.mono44khz"] + ["synth_%02d" % i for i in range(16)] + ["winflags_bcd"]
GATE = 2e-6

# down, up, non-integer ratios, identity; 11025 -> 48000 is the largest LDS table, 44056 -> 16000 needs the global one
PAIRS = [(44100, 16000), (48000, 16000), (16000, 44100), (8000, 16000), (44100, 48000), (48000, 44100), (22050, 16000),
         (11025, 48000), (44056, 16000), (16000, 16000), (24000, 8000)]

pytestmark = pytest.mark.gpu


def _ogg(name):
    return open(os.path.join(GOLDEN, name + ".ogg"), "rb").read()


def _rate(data):
    nseg = data[26]
    return struct.unpack_from("<I", data, 27 + nseg + 12)[0]


def _rehead(data, rate):
    """The same stream with the id header's sample rate rewritten and the first page's CRC recomputed."""
    d = bytearray(data)
    nseg = d[26]
    plen = 27 + nseg + sum(d[27:27 + nseg])
    struct.pack_into("<I", d, 27 + nseg + 12, rate)
    d[22:26] = b"\0\0\0\0"
    struct.pack_into("<I", d, 22, ogg_crc(bytes(d[:plen])))
    return bytes(d)


def _decode_pcm(blobs):
    """ogg_vorbis_decode_corpus, float32 planar: the product's own PCM per file."""
    from parseoggvorbis_amd import pcm
    pcm._load()
    lib = C.CDLL(os.path.join(HOST, "libparseoggvorbis_amd.so"))
    lib.ogg_vorbis_decode_corpus.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_int,
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_char_p)]
    lib.ogg_vorbis_decode_corpus.restype = C.c_int
    n, cap = len(blobs), 131072
    chans = [b[27 + b[26] + 11] for b in blobs]
    datas = (C.c_char_p * n)(*blobs)
    lens = (C.c_size_t * n)(*[len(b) for b in blobs])
    frames, sums, ok = (C.c_uint64 * n)(), (C.c_double * n)(), (C.c_uint8 * n)()
    out = [np.zeros((chans[i], cap), np.float32) for i in range(n)]
    ptrs = (C.c_void_p * n)(*[p.ctypes.data for p in out])
    caps = (C.c_uint64 * n)(*([cap] * n))
    err = C.c_char_p()
    assert lib.ogg_vorbis_decode_corpus(datas, lens, n, 4, 2, 64, 0, frames, sums, ok, ptrs, caps, None, C.byref(err)) == 0, err.value
    assert all(ok)
    return [out[i][:, :frames[i]] for i in range(n)]


def pcm_s16(x):
    return np.clip(np.rint(np.float32(x) * np.float32(32768.0)), -32768, 32767).astype(np.int64)


def check(got, x, r_in, r_out, what):
    """got (C, T_out) float32 against the model over x (C, T); returns the largest |d| / max(1, max|x|)."""
    if rm.ratio(r_in, r_out)[0] == rm.ratio(r_in, r_out)[1]:
        assert np.array_equal(got, x), what
        return 0.0
    want = rm.resample(x, r_in, r_out)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not want.size:
        return 0.0
    scale = max(1.0, float(np.abs(x).max()) if x.size else 0.0)
    e = float(np.abs(got.astype(np.float64) - want).max()) / scale
    assert e <= GATE, (what, e)
    return e


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from parseoggvorbis_amd import pcm, spectral
    return pcm, spectral


@pytest.fixture(scope="module")
def product_pcm(mods):
    blobs = [_ogg(n) for n in FILES]
    return dict(zip(FILES, _decode_pcm(blobs)))


def test_resample_device_against_the_model(mods):
    """(1, 2, 3) vsyn_resample_device on caller buffers: segments of different rates and lengths (0, 1, shorter than the filter,
    thousands) in one call, 1 to 6 channels, every pair of PAIRS (both table variants); frames, sentinels past each segment's
    T_out, and the same bits from a second identical call."""
    import torch
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    rng = np.random.default_rng(17)
    worst = 0.0
    for out_rate, Cn in ((16000, 1), (16000, 2), (44100, 3), (48000, 6)):
        in_rates = [r_in for r_in, r_out in PAIRS if r_out == out_rate] + [44056, 16000, 44100, 0, 8000]
        S, plane = len(in_rates), 7000
        frames = np.array([[7000, 0, 1, 9, 3001, 6999][i % 6] for i in range(S)], np.int32)
        x = (rng.uniform(-1.0, 1.0, (S, Cn, plane)) * (1.0 + 2.0 * (Cn % 2))).astype(np.float32)
        out_plane = max(rm.num_frames(r, out_rate, plane) for r in in_rates if r)
        d_pcm = torch.from_numpy(x).cuda()
        d_frames = torch.from_numpy(frames).cuda()
        results = []
        for rep in range(2):
            d_out = torch.full((S, Cn, out_plane), float("nan"), dtype=torch.float32, device="cuda")
            d_of = torch.full((S,), -1, dtype=torch.int32, device="cuda")
            g.resample_device(in_rates, out_rate, d_pcm.data_ptr(), plane, Cn, d_frames.data_ptr(), d_out.data_ptr(), out_plane,
                              d_of.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            results.append((d_out.cpu().numpy(), d_of.cpu().numpy()))
        (y, of), (y2, of2) = results
        assert np.array_equal(y.view(np.uint32), y2.view(np.uint32)) and np.array_equal(of, of2)  # NaN sentinels compare by bits
        for gi in range(S):
            r_in = in_rates[gi]
            To = rm.num_frames(r_in, out_rate, int(frames[gi])) if r_in else 0
            assert of[gi] == To, (gi, r_in, out_rate, of[gi], To)
            assert np.isnan(y[gi, :, To:]).all(), (gi, r_in, out_rate)  # nothing written past T_out
            if r_in:
                worst = max(worst, check(y[gi, :, :To], x[gi, :, :frames[gi]], r_in, out_rate, (gi, r_in, out_rate, Cn)))
    g.close()
    print("resample_device worst |d| / max(1, max|x|): %.3g" % worst)


def test_resample_device_refuses_bad_arguments(mods):
    import torch
    from parseoggvorbis_amd.binding import Synth, VsynError
    from tests.workloads import fixture_like_spec
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    d = torch.zeros(4096, dtype=torch.float32, device="cuda")
    f = torch.zeros(1, dtype=torch.int32, device="cuda")
    o = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(VsynError, match="100003"):
        g.resample_device([100003], 16000, d.data_ptr(), 100, 1, f.data_ptr(), d.data_ptr(), 4096, o.data_ptr(), s)
    with pytest.raises(VsynError, match="out_plane_stride"):
        g.resample_device([44100], 48000, d.data_ptr(), 1000, 1, f.data_ptr(), d.data_ptr(), 1000, o.data_ptr(), s)
    with pytest.raises(VsynError):
        g.resample_device([44100], 0, d.data_ptr(), 100, 1, f.data_ptr(), d.data_ptr(), 4096, o.data_ptr(), s)
    g.close()


def test_resample_call_leaves_the_pcm_and_the_next_submit_alone(mods):
    """(4) vsyn_pcm_resample_host and vsyn_pcm_resample_spectral_host between two submits: vsyn_pcm_fetch_host and the next
    submit are bit-identical to a handle that made no resample call; f32 and s16 outputs against the model."""
    pcm_mod, spec_mod = mods
    from parseoggvorbis_amd.binding import Synth, VSYN_PCM_F32, VSYN_PCM_S16
    from tests.workloads import fixture_like_spec, synth_batch
    spec = fixture_like_spec(2)
    b1 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=21)
    b2 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=22)
    S = len(b1["segments"])
    rates = [44100, 22050, 48000][:S] + [44100] * max(0, S - 3)
    outs = []
    for with_resample in (False, True):
        g = Synth(spec, device=0, max_streams=4)
        r1 = g.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"], flags=4)  # KEEP_PCM
        assert r1["rc"] == 0
        f1, fr1 = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        if with_resample:
            y, fo = g.pcm_resample_host(rates, 16000, VSYN_PCM_F32)
            y16, fo16 = g.pcm_resample_host(rates, 16000, VSYN_PCM_S16)
            assert np.array_equal(fo, fo16)
            for gi in range(S):
                x = f1[gi, :fr1[gi]].T
                To = rm.num_frames(rates[gi], 16000, int(fr1[gi]))
                assert fo[gi] == To
                check(y[gi, :, :To], x, rates[gi], 16000, ("f32", gi))
                assert not y[gi, :, To:].any()
                want16 = pcm_s16(rm.resample(x, rates[gi], 16000)).T
                assert np.abs(y16[gi, :To].astype(np.int64) - want16).max(initial=0) <= 1, gi
                assert not y16[gi, To:].any()
            kw = dict(kind="log_mel", n_fft=400, hop_length=160, n_mels=40)
            rows = _resample_spectral(g, spec_mod.spectral_spec(**kw), rates, 16000)
            o = 0
            for gi in range(S):
                To = int(fo[gi])
                want, _ = sm.spectral(y[gi, :, :To], 16000, **kw)
                assert rows["seg_rows"][gi] == want.shape[0]
                got = rows["rows"][o:o + want.shape[0]]
                assert np.abs(got.astype(np.float64) - want).max(initial=0) <= 1e-3, gi
                o += want.shape[0]
        f1b, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        assert np.array_equal(f1, f1b)
        r2 = g.submit_host(b2["packets"], b2["segments"], b2["ys"], b2["residue"], b2["plane_stride"])
        assert r2["rc"] == 0
        outs.append((f1, r2["pcm"], r2["emit_len"]))
        g.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])


def _resample_spectral(g, spec, rates, out_rate):
    """vsyn_pcm_resample_spectral_host through the raw library: dict(rows, seg_rows)."""
    from parseoggvorbis_amd.binding import Status
    r = np.ascontiguousarray(rates, np.uint32)
    S = len(r)
    seg = np.zeros(S, np.uint64)
    st, err = Status(), C.c_char_p()
    assert g.lib.vsyn_pcm_resample_spectral_host(g.h, C.byref(spec), S, r.ctypes.data, out_rate, None, 0, seg.ctypes.data, C.byref(st),
                                                 C.byref(err)) == 0, err.value
    total = int(seg.sum())
    rows = np.zeros((max(1, total), spec.n_mels), np.float32)
    assert g.lib.vsyn_pcm_resample_spectral_host(g.h, C.byref(spec), S, r.ctypes.data, out_rate, rows.ctypes.data, total, seg.ctypes.data,
                                                 C.byref(st), C.byref(err)) == 0, err.value
    return dict(rows=rows[:total], seg_rows=seg)


def test_corpus_pcm_against_the_model_over_the_reference_pcm(mods, product_pcm):
    """(5) get_pcm_batch(sr=16000) on every fixture: against the model over the reference decoder's PCM (the PCM gate) and over the
    product's PCM (the device gate); int16 within 1 LSB; sr=None bit for bit what ogg_vorbis_decode_corpus gives."""
    pcm_mod, _ = mods
    blobs = [_ogg(n) for n in FILES]
    res = pcm_mod.get_pcm_batch(blobs, sr=16000)
    res16 = pcm_mod.get_pcm_batch(blobs, sr=16000, dtype="int16")
    native = pcm_mod.get_pcm_batch(blobs)
    worst_ref = worst_dev = 0.0
    for name, data, (y, sr), (y16, sr16), (xn, srn) in zip(FILES, blobs, res, res16, native):
        r_in = _rate(data)
        x = product_pcm[name]
        assert sr == sr16 == 16000 and srn == r_in
        assert xn.dtype == np.float32 and np.array_equal(xn, x), name
        assert y.dtype == np.float32 and y.shape == (x.shape[0], rm.num_frames(r_in, 16000, x.shape[1])), name
        worst_dev = max(worst_dev, check(y, x, r_in, 16000, name))
        ref = np.load(os.path.join(GOLDEN, name + ".npz"))["pcm"]
        want = rm.resample(ref.astype(np.float64), r_in, 16000)
        if want.size:
            worst_ref = max(worst_ref, float(np.abs(y - want).max()) / max(1.0, float(np.abs(ref).max())))
        assert y16.dtype == np.int16 and y16.shape == y.shape[::-1]
        want16 = pcm_s16(rm.resample(x, r_in, 16000)).T
        assert np.abs(y16.astype(np.int64) - want16).max(initial=0) <= 1, name
    print("corpus: |d| / max(1, max|x|) vs model(reference PCM) %.3g, vs model(product PCM) %.3g" % (worst_ref, worst_dev))
    assert worst_ref <= 1e-5
    one = pcm_mod.get_pcm_from_raw_bytes(blobs[0], sr=16000)
    assert one[1] == 16000 and np.array_equal(one[0], res[0][0])


def test_corpus_reheaded_rates_and_a_refused_ratio(mods, product_pcm):
    """(5) one batch of the same stream under four rates: each file is resampled from its own rate; a rate whose reduced ratio
    exceeds the limit (100003 is prime: 16000 / 100003) fails alone, naming the ratio."""
    pcm_mod, _ = mods
    data = _ogg("test.stereo44khz")
    x = product_pcm["test.stereo44khz"]
    rates = [44100, 48000, 22050, 16000, 100003]
    blobs = [data if r == 44100 else _rehead(data, r) for r in rates]
    res = pcm_mod.get_pcm_batch(blobs, sr=16000, errors="return", files_per_submit=8)
    for r, out in zip(rates, res):
        if r == 100003:
            assert isinstance(out, pcm_mod.PcmError) and "16000 / 100003" in str(out), out
            continue
        y, sr = out
        assert sr == 16000
        check(y, x, r, 16000, r)
    assert np.array_equal(res[3][0], x)  # already at 16 kHz: the PCM itself


def test_spectral_with_resampling(mods, product_pcm):
    """(6) get_spectral_batch(sr=16000): the model at 16 kHz over the resampled PCM; a 16 kHz file gives the same bits with
    sr=16000 and sr=None; a mixed-rate batch uses one 16 kHz mel table, and fmin / fmax are checked against 16 kHz."""
    pcm_mod, spec_mod = mods
    data = _ogg("test.stereo44khz")
    blobs = [data, _rehead(data, 48000), _rehead(data, 22050), _rehead(data, 16000), _ogg("synth_03"), _ogg("test.mono44khz")]
    pcm16k = pcm_mod.get_pcm_batch(blobs, sr=16000)
    for kw in (dict(kind="log_mel", n_fft=400, hop_length=160, n_mels=40), dict(kind="mel_power", n_fft=512, hop_length=128, n_mels=64)):
        res = spec_mod.get_spectral_batch(blobs, sr=16000, **kw)
        for i, (got, (y, sr)) in enumerate(zip(res, pcm16k)):
            want, M = sm.spectral(y, 16000, **kw)
            assert got.shape == want.shape, (i, kw)
            if not want.size:
                continue
            d = np.abs(got.astype(np.float64) - want)
            tol = 1e-3 if kw["kind"] == "log_mel" else 1e-5 * np.abs(want).max()
            assert (d <= tol).all(), (i, kw, float(d.max()))
        if kw["kind"] == "mel_power":  # against the model chain over the product PCM: resampling error stays inside the gate
            for i, name in ((0, "test.stereo44khz"), (4, "synth_03"), (5, "test.mono44khz")):
                want, _ = sm.spectral(rm.resample(product_pcm[name], _rate(blobs[i]), 16000), 16000, **kw)
                assert np.abs(res[i] - want).max() <= 1e-5 * np.abs(want).max(), i
        low = spec_mod.get_spectral_batch([blobs[3]], **kw)[0]
        assert np.array_equal(spec_mod.get_spectral_from_raw_bytes(blobs[3], sr=16000, **kw), low)
        assert np.array_equal(res[3], low)
    bad = spec_mod.get_spectral_batch(blobs[:2], sr=16000, errors="return", kind="log_mel", n_fft=400, hop_length=160, n_mels=40,
                                      fmax=11025.0)
    assert all(isinstance(r, spec_mod.SpectralError) and "16000" in str(r) for r in bad)


@pytest.mark.parametrize("run", ["pcm-float32", "pcm-int16", "spectral"])
@pytest.mark.parametrize("sr", [None, 16000])
def test_refused_file_fails_alone_in_a_batch(run, sr):
    """winflags_a is refused by the synthesis layer; in one submit with three winflags_bcd files (same setup, one
    feeder, so all four share the submit) the flagged batch is re-run file by file: five submits. Only file 1 fails, naming the
    condition; every other entry is bit for bit that file's result alone."""
    from parseoggvorbis_amd import pcm, spectral
    names = ["winflags_bcd", "winflags_a", "winflags_bcd", "winflags_bcd"]
    blobs = [_ogg(n) for n in names]
    stats = []
    if run == "spectral":
        err_cls = spectral.SpectralError
        res = spectral.get_spectral_batch(blobs, sr=sr, feeders=1, files_per_submit=4, errors="return", stats=stats)
        alone = [spectral.get_spectral_batch([b], sr=sr, errors="return")[0] for b in blobs]
        arrays = lambda r: [r]  # noqa: E731
    else:
        err_cls = pcm.PcmError
        dtype = run.split("-")[1]
        res = pcm.get_pcm_batch(blobs, sr=sr, dtype=dtype, feeders=1, files_per_submit=4, errors="return", stats=stats)
        alone = [pcm.get_pcm_batch([b], sr=sr, dtype=dtype, errors="return")[0] for b in blobs]
        arrays = lambda r: [r[0], np.int64(r[1])]  # noqa: E731
    assert stats[5] == 5, stats  # the flagged 4-file submit, then one per file
    for i, (got, want) in enumerate(zip(res, alone)):
        if i == 1:
            assert isinstance(got, err_cls) and "file 1" in str(got) and "window-flags" in str(got), str(got)
            continue
        assert not isinstance(got, Exception) and not isinstance(want, Exception), (i, str(got), str(want))
        for a, b in zip(arrays(got), arrays(want)):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), i
