"""PCM conditioning on the GPU (vsyn_pcm_condition_device, vsyn_pcm_condition_host, vsyn_pcm_cond_spectral_host,
ogg_vorbis_pcm_corpus_cond, ogg_vorbis_spectral_corpus_cond, get_pcm_batch(mono=, peak_normalize=, preemphasis=),
get_spectral_batch(peak_normalize=, preemphasis=)) against the float64 model of tests/condition_model.py.

Gates of the stage alone, from the arithmetic the device uses, u = 2^-24:
    downmix       C - 1 float32 additions, the rounding of 1 / C and one multiplication:
                  |d| <= (C + 1) u (1 / C) sum_c |x_c[t]| against the float64 mean; C = 1 is the input, bit for bit.
    peak          the returned p equals max |y| of the device's own downmix plane exactly, and y1 equals numpy's float32 y / p bit
                  for bit (both are the correctly rounded division).
    pre-emphasis  one FMA rounding: |d| <= u |z64|, z64 = y1[t] - a32 y1[t-1] in float64 on the device's own y1.
The peak and pre-emphasis checks run the model on the device's own downmix plane (fetched with both options off), as the post-stage
tests isolate their stage. Measured on the MI355X, worst |d| / bound over test_stage_alone_against_the_model: see that test's
docstring. End to end the gate is GATE of tests/test_gpu_spectral.py, unchanged, on the device's own conditioned plane as 1-channel
input: see test_conditioned_spectral_rows_equal_the_model's docstring for the measured ratios.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from tests import condition_model as cm
from tests.test_gpu_spectral import FILES, GATE, _decode_pcm, _ogg, _rate, assert_matches
from tests.test_gpu_spectral_post import E2E, _compare_batch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
A = 0.97
A32 = cm.coefficient(A)
TS = [0, 1, 2, 63, 64, 65, 4097, 100003]


def _cond(peak=False, a=None):
    from parseoggvorbis_amd.binding import PcmCond
    return PcmCond((1 if peak else 0) | (2 if a is not None else 0), 0, 0.0 if a is None else float(np.float32(a)))


@pytest.fixture(scope="module")
def synth():
    import torch
    assert torch.cuda.is_available()
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    yield g
    g.close()


def _run_stage(g, cond, x, frames, out_plane=None, in_off=0, out_off=0):
    """vsyn_pcm_condition_device over x (S, C, plane) float32 with frames [S]; the input starts in_off floats, the output out_off
    floats behind a 16-byte boundary. Returns (out (S, out_plane) float32, NaN where nothing was written; peaks (S,) float32, NaN
    where nothing was written)."""
    import torch
    S, Cn, plane = x.shape
    out_plane = plane if out_plane is None else out_plane
    buf = torch.zeros(x.size + 8, dtype=torch.float32, device="cuda")
    buf[in_off:in_off + x.size].copy_(torch.from_numpy(np.ascontiguousarray(x).ravel()))
    d_frames = torch.from_numpy(np.asarray(frames, np.int32)).cuda()
    d_out = torch.full((S * out_plane + 8,), float("nan"), dtype=torch.float32, device="cuda")
    d_peaks = torch.full((S,), float("nan"), dtype=torch.float32, device="cuda")
    g.pcm_condition_device(cond, buf.data_ptr() + 4 * in_off, plane, Cn, S, d_frames.data_ptr(), d_out.data_ptr() + 4 * out_off, out_plane,
                           d_peaks.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    flat = d_out.cpu().numpy()
    assert np.isnan(flat[:out_off]).all() and np.isnan(flat[out_off + S * out_plane:]).all()
    return flat[out_off:out_off + S * out_plane].reshape(S, out_plane), d_peaks.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _planes(rng, Cn, plane):
    """One batch: the eight lengths of TS, an all-zero segment and a segment whose peak is its last sample."""
    frames = TS + [5000, 777]
    x = (rng.standard_normal((len(frames), Cn, plane)) * 0.2).astype(np.float32)
    x[8] = 0.0
    x[9, :, 776] = np.float32(3.0) + np.arange(Cn, dtype=np.float32)
    return x, frames


def test_stage_alone_against_the_model(synth):
    """C = 1 .. 6, T in TS, an odd plane stride (4-byte loads) and a multiple of 4 with the planes 0 .. 3 floats off a 16-byte
    boundary (16-byte loads with a scalar head and tail), frames < plane_stride, output stride != input stride.
    Measured on the MI355X: worst downmix |d| / bound 0.696, worst pre-emphasis |d| / (u |z64|) 1.000 (the unit roundoff of the one
    FMA rounding); peaks and y1 exact."""
    rng = np.random.default_rng(2025)
    worst_mix, worst_pre = 0.0, 0.0
    for Cn in range(1, 7):
        for plane, in_off, out_off in ((100007, 0, 0), (100004, 0, 0), (100004, 1, 3), (100004, 2, 0), (100004, 3, 1)):
            x, frames = _planes(rng, Cn, plane)
            S = len(frames)
            out_plane = plane + 5
            y, pk0 = _run_stage(synth, _cond(), x, frames, out_plane, in_off, out_off)
            assert np.isnan(pk0).all()  # not written without VSYN_COND_PEAK
            yp, pk = _run_stage(synth, _cond(True), x, frames, out_plane, in_off, out_off)
            ypre, _ = _run_stage(synth, _cond(False, A), x, frames, out_plane, in_off, out_off)
            z, pk2 = _run_stage(synth, _cond(True, A), x, frames, out_plane, in_off, out_off)
            assert np.array_equal(_bits(pk), _bits(pk2))
            for gi, T in enumerate(frames):
                what = (Cn, plane, in_off, gi, T)
                for out in (y, yp, ypre, z):
                    assert np.isnan(out[gi, T:]).all() and not np.isnan(out[gi, :T]).any(), what  # nothing past T, all of it below
                x64 = x[gi, :, :T].astype(np.float64)
                yg = y[gi, :T]
                if Cn == 1:
                    assert np.array_equal(_bits(yg), _bits(x[gi, 0, :T])), what
                else:  # the downmix against the float64 mean
                    bound = (Cn + 1) * U * np.abs(x64).sum(axis=0) / Cn
                    d = np.abs(yg.astype(np.float64) - cm.downmix(x64))
                    assert (d <= bound).all(), (what, float((d / np.maximum(bound, 1e-300)).max()))
                    if T and bound.max() > 0:
                        worst_mix = max(worst_mix, float((d[bound > 0] / bound[bound > 0]).max()))
                # the peak: max |y| exactly; y1 = numpy's float32 division, bit for bit
                p = np.abs(yg).max() if T else np.float32(0.0)
                assert _bits(pk[gi]) == _bits(p), (what, pk[gi], p)
                assert p == np.float32(cm.peak(yg))
                y1 = yg / p if p > 0 else yg
                assert y1.dtype == np.float32 and np.array_equal(_bits(yp[gi, :T]), _bits(y1)), what
                if p > 0:
                    assert np.abs(yp[gi, :T]).max() == np.float32(1.0), what
                else:
                    assert not yp[gi, :T].any() and not z[gi, :T].any(), what  # silence stays silence
                if gi == 9:
                    assert np.abs(yg[-1]) == p  # the segment whose peak is its last sample
                # the pre-emphasis: one FMA rounding on the device's own y1 (with the peak) and y (without)
                for got, src in ((z[gi, :T], y1), (ypre[gi, :T], yg)):
                    z64 = cm.preemphasis(src.astype(np.float64), A)
                    d = np.abs(got.astype(np.float64) - z64)
                    bound = U * np.abs(z64)
                    assert (d <= bound).all(), (what, float((d / np.maximum(bound, 1e-300)).max()))
                    if T:
                        assert _bits(got[0]) == _bits(src[0])
                        nz = bound > 0
                        if nz.any():
                            worst_pre = max(worst_pre, float((d[nz] / bound[nz]).max()))
            assert S == 10
    print("stage alone: worst downmix |d| / bound %.3f, worst pre-emphasis |d| / (u |z64|) %.3f" % (worst_mix, worst_pre))


def test_exact_properties(synth):
    """No tolerance: the peak becomes exactly 1; 2^k x gives the bits of x under peak normalisation; a segment gives the same bits
    whatever its slot, its neighbours and the planes' alignment; two runs give the same bits."""
    rng = np.random.default_rng(11)
    for Cn in (1, 2, 3, 6):
        plane = 100004
        x, frames = _planes(rng, Cn, plane)
        for cond in (_cond(True), _cond(True, A)):
            base, pk = _run_stage(synth, cond, x, frames)
            again, _ = _run_stage(synth, cond, x, frames)
            assert np.array_equal(_bits(base), _bits(again))
            for k in (3, -3):
                sc, pks = _run_stage(synth, cond, x * np.float32(2.0 ** k), frames)
                assert np.array_equal(_bits(sc), _bits(base)), (Cn, k)
                assert np.array_equal(_bits(pks), _bits(pk * np.float32(2.0 ** k)))
            if not cond.options & 2:
                for gi, T in enumerate(frames):
                    if T and gi != 8:
                        assert np.abs(base[gi, :T]).max() == np.float32(1.0), (Cn, gi)
            # slot and neighbours: segment 7 alone, and as the first of three in another order
            alone, pa = _run_stage(synth, cond, x[7:8], frames[7:8])
            assert np.array_equal(_bits(alone[0]), _bits(base[7])) and _bits(pa[0]) == _bits(pk[7])
            order = [7, 9, 3]
            mixed, pm_ = _run_stage(synth, cond, x[order], [frames[i] for i in order])
            for j, i in enumerate(order):
                assert np.array_equal(_bits(mixed[j]), _bits(base[i])) and _bits(pm_[j]) == _bits(pk[i]), (Cn, i)
            # the planes' alignment: 4-byte loads (odd stride), 16-byte loads with a head (offset 1 .. 3) — same bits
            odd = np.zeros((len(frames), Cn, plane + 3), np.float32)
            odd[:, :, :plane] = x
            o, po = _run_stage(synth, cond, odd, frames)
            assert np.array_equal(_bits(o[:, :plane]), _bits(base)) and np.array_equal(_bits(po), _bits(pk))
            for off in (1, 2, 3):
                o, po = _run_stage(synth, cond, x, frames, None, off, (off + 1) & 3)
                assert np.array_equal(_bits(o), _bits(base)) and np.array_equal(_bits(po), _bits(pk)), (Cn, off)


def test_a_segment_that_is_not_finite_is_refused_alone(synth):
    """An Inf (or NaN) sample: that segment's peak word says so and its plane is zeros; its neighbours' outputs and peaks equal
    those of a run without the sample. Without VSYN_COND_PEAK nothing is checked and the sample passes through."""
    rng = np.random.default_rng(5)
    for Cn, bad_value in ((2, np.inf), (3, -np.inf), (1, np.nan), (2, np.nan)):
        x, frames = _planes(rng, Cn, 100004)
        bad = x.copy()
        bad[6, Cn - 1, 4000] = bad_value
        for cond in (_cond(True), _cond(True, A)):
            want, pw = _run_stage(synth, cond, x, frames)
            got, pg = _run_stage(synth, cond, bad, frames)
            refused = [gi for gi in range(len(frames)) if not np.isfinite(pg[gi])]
            assert refused == [6], (Cn, bad_value, pg)  # by name: segment 6 and no other
            assert not got[6, :frames[6]].any() and np.isnan(got[6, frames[6]:]).all()
            for gi in range(len(frames)):
                if gi != 6:
                    assert np.array_equal(_bits(got[gi]), _bits(want[gi])) and _bits(pg[gi]) == _bits(pw[gi]), (Cn, gi)
        passed, _ = _run_stage(synth, _cond(), bad, frames)
        assert not np.isfinite(passed[6, 4000]) and np.isfinite(passed[6, :4000]).all()


def test_stage_refuses_bad_arguments(synth):
    from parseoggvorbis_amd.binding import PcmCond, VsynError
    x = np.zeros((1, 2, 64), np.float32)
    for cond in (PcmCond(4, 0, 0.0), PcmCond(2, 0, 0.0), PcmCond(2, 0, 1.0), PcmCond(2, 0, -0.5), PcmCond(2, 0, float("nan")),
                 PcmCond(3, 0, float("inf")), PcmCond(2, 0, 1.0 - 1e-12)):
        with pytest.raises(VsynError) as ei:
            _run_stage(synth, cond, x, [64])
        assert ei.value.code == 1, str(ei.value)  # VSYN_ERR_INVALID
    import torch
    t = torch.zeros(256, dtype=torch.float32, device="cuda")
    f = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(VsynError) as ei:  # channels = 0
        synth.pcm_condition_device(_cond(), t.data_ptr(), 64, 0, 1, f.data_ptr(), t.data_ptr(), 64)
    assert ei.value.code == 1
    assert _run_stage(synth, PcmCond(1, 0, 7.0), x, [64])[0].shape == (1, 64)  # the coefficient is not read without its option


# ---- end to end on the committed fixtures ----

@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from parseoggvorbis_amd import pcm, spectral
    return pcm, spectral


@pytest.fixture(scope="module")
def blobs():
    return [_ogg(n) for n in FILES]


@pytest.fixture(scope="module")
def pcm_by_rate(mods, blobs):
    """The product's own C-channel PCM per fixture: at each file's rate (None, ogg_vorbis_decode_corpus) and resampled on the device
    to 16 kHz (the existing get_pcm_batch(sr=16000))."""
    native = _decode_pcm(blobs)
    low = [y for y, _ in mods[0].get_pcm_batch(blobs, sr=16000)]
    return {None: dict(zip(FILES, native)), 16000: dict(zip(FILES, low))}


def _stage_on_file(g, cond, x):
    """The stage alone on one file's (C, T) PCM: the (T,) plane."""
    T = x.shape[1]
    xs = np.zeros((1, x.shape[0], max(T, 1)), np.float32)
    xs[0, :, :T] = x
    out, pk = _run_stage(g, cond, xs, [T])
    return out[0, :T], pk[0]


def _s16(plane):
    """ov_read's conversion (vsyn_pcm_interleave_device): the float32 product x * 32768 rounded to the nearest-even integer, clamped."""
    return np.clip(np.rint(plane.astype(np.float32) * np.float32(32768.0)), -32768.0, 32767.0).astype(np.int16)


def test_stage_off_means_off(mods, blobs, pcm_by_rate):
    """The new arguments at their defaults, and the new corpus entries with a NULL cond, give the existing entry points' bits."""
    pcm, spectral = mods
    from parseoggvorbis_amd import _corpus
    lib = pcm._load()
    n = len(blobs)
    for sr in (None, 16000):
        got = pcm.get_pcm_batch(blobs, sr=sr, mono=False, peak_normalize=False, preemphasis=None)
        for name, (y, r) in zip(FILES, got):
            want = pcm_by_rate[sr][name]
            assert y.shape == want.shape and np.array_equal(_bits(y), _bits(want)), (name, sr)
        # ogg_vorbis_pcm_corpus_cond with cond = NULL
        for dtype, fmt in (("float32", 2), ("int16", 1)):
            frames, chans, rates = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)

            def build(i, p):
                T, Cn = int(frames[i]), int(chans[i])
                a = np.zeros((Cn, T), np.float32) if fmt == 2 else np.zeros((T, Cn), np.int16)
                return _corpus.copy_into(a, p)

            via_new = _corpus.run(lib, lib.ogg_vorbis_pcm_corpus_cond, blobs, (4, 2, 64, 0, sr or 0, fmt, None), (frames, chans, rates),
                                  build, pcm.PcmError, "raise", "pcm")
            old = pcm.get_pcm_batch(blobs, sr=sr, dtype=dtype)
            for a, (b, _) in zip(via_new, old):
                assert a.shape == b.shape and np.array_equal(a, b)
        for kw in (E2E[0], E2E[1]):
            a = spectral.get_spectral_batch(blobs, sr=sr, **kw)
            b = spectral.get_spectral_batch(blobs, sr=sr, peak_normalize=False, preemphasis=None, **kw)
            spec = spectral.spectral_spec(**kw)
            counts = np.zeros(n, np.uint64)
            dim = spectral.spec_dim(spec)
            c = _corpus.run(lib, lib.ogg_vorbis_spectral_corpus_cond, blobs, (4, 2, 64, 0, C.byref(spec), sr or 0, None, None), (counts,),
                            lambda i, p: _corpus.copy_into(np.zeros((int(counts[i]), dim), np.float32), p), spectral.SpectralError, "raise",
                            "spectral")
            for p, q, r in zip(a, b, c):
                assert np.array_equal(_bits(p), _bits(q)) and p.shape == r.shape and np.array_equal(_bits(p), _bits(r))


def test_mono_pcm_equals_the_stage_alone(mods, blobs, pcm_by_rate, synth):
    """get_pcm_batch(mono=True, ...): (frames,) float32 equal to the stage alone on that file's decoded (resampled) PCM, bit for
    bit; int16 equal to the existing conversion of that plane, and for the 1-channel fixtures to the existing int16 entry."""
    pcm, _ = mods
    for sr in (None, 16000):
        old16 = pcm.get_pcm_batch(blobs, sr=sr, dtype="int16")
        for peak, a in ((False, None), (True, None), (False, A), (True, A)):
            f32 = pcm.get_pcm_batch(blobs, sr=sr, mono=True, peak_normalize=peak, preemphasis=a)
            s16 = pcm.get_pcm_batch(blobs, sr=sr, dtype="int16", mono=True, peak_normalize=peak, preemphasis=a)
            for i, (name, data) in enumerate(zip(FILES, blobs)):
                x = pcm_by_rate[sr][name]
                y, r = f32[i]
                assert r == (sr or _rate(data)) and s16[i][1] == r
                assert y.dtype == np.float32 and y.shape == (x.shape[1],), (name, y.shape)
                want, _ = _stage_on_file(synth, _cond(peak, a), x)
                assert np.array_equal(_bits(y), _bits(want)), (name, sr, peak, a)
                q = s16[i][0]
                assert q.dtype == np.int16 and q.shape == (x.shape[1],)
                assert np.array_equal(q, _s16(y)), (name, sr, peak, a)
                if x.shape[0] == 1 and not peak and a is None:
                    assert np.array_equal(q, old16[i][0][:, 0]) and np.array_equal(_bits(y), _bits(x[0])), name
                if peak and a is None and y.size and np.abs(y).max() > 0:
                    assert np.abs(y).max() == np.float32(1.0), name
    one = pcm.get_pcm_from_raw_bytes(blobs[0], mono=True, peak_normalize=True, preemphasis=A)
    assert np.array_equal(_bits(one[0]), _bits(pcm.get_pcm_batch(blobs, mono=True, peak_normalize=True, preemphasis=A)[0][0]))


def test_the_mono_plane_gives_todays_rows_bit_for_bit(mods, blobs, synth):
    """The shared downmix: the mono plane of get_pcm_batch(mono=True) given to vsyn_spectral_device as 1-channel PCM gives the rows
    get_spectral_batch gives on the C-channel PCM, bit for bit."""
    import torch
    pcm, spectral = mods
    for sr in (None, 16000):
        planes = pcm.get_pcm_batch(blobs, sr=sr, mono=True)
        for kw in (E2E[0], E2E[1], dict(kind="mel_power", n_fft=512, hop_length=128, n_mels=32, power=1)):
            want = spectral.get_spectral_batch(blobs, sr=sr, **kw)
            s = spectral.spectral_spec(**kw)
            dim = spectral.spec_dim(s)
            for name, (y, r), w in zip(FILES, planes, want):
                T = y.shape[0]
                d_pcm = torch.from_numpy(np.ascontiguousarray(y) if T else np.zeros(1, np.float32)).cuda()
                d_frames = torch.tensor([T], dtype=torch.int32, device="cuda")
                d_rows = torch.full((w.shape[0] + 2, dim), float("nan"), dtype=torch.float32, device="cuda")
                d_off = torch.zeros(2, dtype=torch.int64, device="cuda")
                synth.spectral_device(s, [r], d_pcm.data_ptr(), max(T, 1), 1, d_frames.data_ptr(), d_rows.data_ptr(), d_off.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert int(d_off.cpu()[1]) == w.shape[0], (name, sr)
                assert np.array_equal(_bits(d_rows.cpu().numpy()[:w.shape[0]]), _bits(w)), (name, sr, kw["kind"])


def test_conditioned_spectral_rows_equal_the_model(mods, blobs):
    """get_spectral_batch(peak_normalize=True, preemphasis=0.97) for the three specs of E2E, at the native rate and at 16 kHz, against
    tests/spectral_model.py run on the device's own conditioned plane (get_pcm_batch(mono=True, peak_normalize=True,
    preemphasis=0.97)) under GATE of tests/test_gpu_spectral.py, unchanged; then one case with delta=2, normalize="mean_var" on top
    under the post tests' composed gate.
    Measured on the MI355X, worst |d| / gate per kind: log_mel 0.0008, mfcc 0.0142, mel_db 0.1418; with delta 2 / mean_var on top
    (log_mel, ratio to the composed gate): 0.0004 at the native rate, 0.0003 at 16 kHz. No kind comes near its gate on
    pre-emphasised input: the peak-normalised, pre-emphasised fixtures have little energy, so log_mel sits at its floor (1e-3) on
    most bands."""
    pcm, spectral = mods
    worst = {}
    for sr in (None, 16000):
        planes = pcm.get_pcm_batch(blobs, sr=sr, mono=True, peak_normalize=True, preemphasis=A)
        for kw in E2E:
            res = spectral.get_spectral_batch(blobs, sr=sr, peak_normalize=True, preemphasis=A, **kw)
            for name, (y, r), got in zip(FILES, planes, res):
                e = assert_matches(got, y[None, :], r, kw, (name, sr, kw))
                worst[kw["kind"]] = max(worst.get(kw["kind"], 0.0), e / GATE[kw["kind"]])
        # the chain in the stated order: condition, STFT, then the post stage
        shim = types.SimpleNamespace(get_spectral_batch=functools.partial(spectral.get_spectral_batch, peak_normalize=True, preemphasis=A),
                                     SpectralError=spectral.SpectralError)
        as_pcm = {sr: {name: y[None, :] for name, (y, _) in zip(FILES, planes)}}
        n, w = _compare_batch(shim, as_pcm, E2E[0], 2, 9, "mean_var", sr)
        assert n > 0
        worst["post/%s" % sr] = w
    print("end to end, worst |d| / gate:", {k: round(v, 4) for k, v in sorted(worst.items())})


def test_host_entries_leave_the_pcm_and_the_next_submit_alone(mods, synth):
    """vsyn_pcm_condition_host and vsyn_pcm_cond_spectral_host between two submits: vsyn_pcm_fetch_host and the next submit are
    bit-identical to a handle that made no such call; their outputs equal the stage alone on the fetched PCM (resampled: the frame
    counts), and a NULL cond gives the existing entry point's rows."""
    from parseoggvorbis_amd.binding import Synth, VSYN_PCM_F32, VSYN_PCM_S16
    from tests.workloads import fixture_like_spec, synth_batch
    _, spectral = mods
    spec = fixture_like_spec(2)
    b1 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=11)
    b2 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=12)
    S = len(b1["segments"])
    outs = []
    for with_cond in (False, True):
        g = Synth(spec, device=0, max_streams=4)
        r1 = g.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"], flags=4)  # KEEP_PCM
        assert r1["rc"] == 0
        f1, fr1 = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        if with_cond:
            s = spectral.spectral_spec(kind="log_mel", n_fft=400, hop_length=160, n_mels=40)
            plain = g.pcm_spectral_host(s, [44100] * S)
            off = g.pcm_cond_spectral_host(None, s, None, [44100] * S)
            assert np.array_equal(_bits(off["rows"]), _bits(plain["rows"])) and np.array_equal(off["seg_rows"], plain["seg_rows"])
            assert not off["peaks"].any()
            for cond in (_cond(), _cond(True, A)):
                out, frames, peaks = g.pcm_condition_host(cond, S)
                out16, frames16, _ = g.pcm_condition_host(cond, S, fmt=VSYN_PCM_S16)
                assert np.array_equal(frames, fr1) and np.array_equal(frames16, fr1)
                rows = g.pcm_cond_spectral_host(cond, s, None, [44100] * S)
                assert rows["rc"] == 0 and np.array_equal(_bits(rows["peaks"]), _bits(peaks))
                o = 0
                for gi in range(S):
                    T = int(fr1[gi])
                    want, pk = _stage_on_file(synth, cond, np.ascontiguousarray(f1[gi, :T].T))
                    assert np.array_equal(_bits(out[gi, :T]), _bits(want)) and not out[gi, T:].any(), gi
                    assert np.array_equal(out16[gi, :T], _s16(want)) and not out16[gi, T:].any(), gi
                    if cond.options & 1:
                        assert _bits(peaks[gi]) == _bits(pk)
                    nr = int(rows["seg_rows"][gi])
                    assert_matches(rows["rows"][o:o + nr], want[None, :], 44100, dict(kind="log_mel", n_fft=400, hop_length=160, n_mels=40),
                                   ("host", gi))
                    o += nr
                rs, frs, _ = g.pcm_condition_host(cond, S, [44100] * S, 16000)
                assert rs.shape[0] == S and (frs == [-(-int(t) * 160 // 441) for t in fr1]).all()
        f1b, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        assert np.array_equal(f1, f1b)
        r2 = g.submit_host(b2["packets"], b2["segments"], b2["ys"], b2["residue"], b2["plane_stride"])
        assert r2["rc"] == 0
        outs.append((f1, r2["pcm"], r2["emit_len"]))
        g.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])


def test_full_chain_equals_the_stages_one_by_one(mods, synth):
    """Stage chaining, no tolerance: the rows, seg_rows and peaks of one vsyn_pcm_cond_spectral_host call (resample, condition, STFT /
    mel, post) equal those of vsyn_resample_device -> vsyn_pcm_condition_device -> vsyn_spectral_device -> vsyn_spectral_post_device
    run one by one on the fetched PCM, on planes of another stride (t_max + 5) than the host form's (t_max); and the PCM of
    vsyn_pcm_condition_host, F32 and S16, equals that run's conditioned plane. Three segments at 8000 (resampled 1:2), 16000 (ratio 1)
    and 0 Hz (skipped: 0 frames, 0 rows, peak 0); the longest segment is the one resampled 1:2, so that a plane of t_max + 5 frames
    holds every input plane resampled, which vsyn_resample_device asks for."""
    import torch
    from parseoggvorbis_amd.binding import Synth, VSYN_PCM_F32, VSYN_PCM_S16
    from tests.workloads import fixture_like_spec, synth_batch
    _, spectral = mods
    spec = fixture_like_spec(2)
    b = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=21)
    S, Cn, rates, out_rate = len(b["segments"]), 2, [16000, 0, 8000], 16000
    assert S == 3
    cond = _cond(True, A)
    s = spectral.spectral_spec(kind="mel_db", n_fft=64, hop_length=32, n_mels=8)
    dim = spectral.spec_dim(s)
    post, dout, _ = spectral.post_spec(dim, delta=1, delta_width=3, normalize="mean_var")
    g = Synth(spec, device=0, max_streams=4)
    try:
        assert g.submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"], flags=4)["rc"] == 0  # KEEP_PCM
        f1, fr = g.pcm_fetch_host(VSYN_PCM_F32, S, b["plane_stride"])
        host = g.pcm_cond_spectral_host(cond, s, post, rates, out_rate)
        out32, frames32, peaks32 = g.pcm_condition_host(cond, S, rates, out_rate)
        out16, frames16, peaks16 = g.pcm_condition_host(cond, S, rates, out_rate, fmt=VSYN_PCM_S16)
    finally:
        g.close()
    assert host["rc"] == 0
    T = [int(t) * out_rate // r if r else 0 for t, r in zip(fr, rates)]
    t_max = max(T)
    assert T[0] > 0 and T[2] == 2 * int(fr[2]) and list(frames32) == T and list(frames16) == T
    plane = t_max + 5                # of the resampled and of the conditioned planes
    in_plane = plane // 2            # vsyn_resample_device wants room for a whole input plane resampled
    assert int(fr.max()) <= in_plane
    x = np.zeros((S, Cn, in_plane), np.float32)
    for gi in range(S):
        x[gi, :, :int(fr[gi])] = f1[gi, :int(fr[gi])].T
    st = torch.cuda.current_stream().cuda_stream
    d_x = torch.from_numpy(x).cuda()
    d_fr = torch.from_numpy(fr.astype(np.int32)).cuda()
    d_rs = torch.full((S * Cn * plane,), float("nan"), dtype=torch.float32, device="cuda")
    d_rsf = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    synth.resample_device(rates, out_rate, d_x.data_ptr(), in_plane, Cn, d_fr.data_ptr(), d_rs.data_ptr(), plane, d_rsf.data_ptr(), st)
    d_cd = torch.full((S * plane,), float("nan"), dtype=torch.float32, device="cuda")
    d_pk = torch.full((S,), float("nan"), dtype=torch.float32, device="cuda")
    synth.pcm_condition_device(cond, d_rs.data_ptr(), plane, Cn, S, d_rsf.data_ptr(), d_cd.data_ptr(), plane, d_pk.data_ptr(), st)
    n_rows = [int(synth.lib.vsyn_spectral_num_frames(C.byref(s), t)) if r else 0 for t, r in zip(T, rates)]
    total = sum(n_rows)
    d_rows = torch.full((total + 2, dim), float("nan"), dtype=torch.float32, device="cuda")
    d_off = torch.full((S + 1,), -1, dtype=torch.int64, device="cuda")
    synth.spectral_device(s, [out_rate if r else 0 for r in rates], d_cd.data_ptr(), plane, 1, d_rsf.data_ptr(), d_rows.data_ptr(),
                          d_off.data_ptr(), st)
    d_post = torch.full((total + 2, dout), float("nan"), dtype=torch.float32, device="cuda")
    synth.spectral_post_device(post, dim, n_rows, d_rows.data_ptr(), d_post.data_ptr(), st)
    torch.cuda.synchronize()
    assert list(d_rsf.cpu().numpy()) == T
    off = d_off.cpu().numpy()
    assert list(np.diff(off)) == n_rows and off[0] == 0
    # the rows, seg_rows and peaks of the one host call
    assert list(host["seg_rows"]) == n_rows and n_rows[1] == 0 and min(n_rows[0], n_rows[2]) >= 3
    want_rows = d_post.cpu().numpy()
    assert np.isnan(want_rows[total:]).all() and not np.isnan(want_rows[:total]).any()
    assert host["rows"].shape == (total, dout) and np.array_equal(_bits(host["rows"]), _bits(want_rows[:total]))
    pk = d_pk.cpu().numpy()
    assert pk[1] == 0 and pk[0] > 0 and pk[2] > 0
    assert np.array_equal(_bits(host["peaks"]), _bits(pk))
    # the PCM of vsyn_pcm_condition_host
    cd = d_cd.cpu().numpy().reshape(S, plane)
    assert np.array_equal(_bits(peaks32), _bits(pk)) and np.array_equal(_bits(peaks16), _bits(pk))
    assert out32.shape == (S, t_max) and out16.shape == (S, t_max)
    for gi in range(S):
        assert np.isnan(cd[gi, T[gi]:]).all() and not np.isnan(cd[gi, :T[gi]]).any(), gi
        assert np.array_equal(_bits(out32[gi, :T[gi]]), _bits(cd[gi, :T[gi]])) and not out32[gi, T[gi]:].any(), gi
        assert np.array_equal(out16[gi, :T[gi]], _s16(cd[gi, :T[gi]])) and not out16[gi, T[gi]:].any(), gi
