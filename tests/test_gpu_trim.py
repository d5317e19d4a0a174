"""PCM trimming on the GPU (vsyn_pcm_trim_device, vsyn_pcm_trim_host, vsyn_pcm_trim_spectral_host, ogg_vorbis_pcm_corpus_trim,
ogg_vorbis_spectral_corpus_trim, get_pcm_batch(trim_db=, ...), get_spectral_batch(trim_db=, ...)) against the float64 model of
tests/trim_model.py.

Gates of the stage alone:
    ms[f]         one float64 chain of L non-negative terms and the division: |d| <= (L + 1) * 2^-53 * ms[f].
    R             max(ms) of the device's own d_ms (or 1e-10), exactly.
    (start, end)  the model's, on inputs whose model margin is above (2L + 3) * 2^-53 (asserted here and, without a GPU, in
                  tests/test_trim_cpu.py).
    plane         the stage's own downmix (the conditioning stage with options = 0) sliced [start:end], bit for bit.
End to end the truth is the model on the device's own mono plane, and for the rows GATE of tests/test_gpu_spectral.py, unchanged.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from tests import trim_cases as tc
from tests import trim_model as tm
from tests.test_gpu_condition import A, _bits, _cond, _run_stage, _s16, _stage_on_file, blobs, mods, pcm_by_rate, synth  # noqa: F401
from tests.test_gpu_spectral import FILES, GATE, _rate, assert_matches
from tests.test_gpu_spectral_post import E2E, _compare_batch

pytestmark = pytest.mark.gpu

E2E_TRIM = [(60.0, 2048, 512), (40.0, 400, 160), (20.0, 64, 16)]
# (odd plane stride, input offset, output offset in floats from a 16-byte boundary): the strides and offsets of the conditioning
# stage's per-value test
VARIANTS = [(True, 0, 0), (False, 0, 0), (False, 1, 3), (False, 2, 0), (False, 3, 1)]


def _trim(top_db=60.0, L=2048, H=512):
    from parseoggvorbis_amd.binding import PcmTrim
    return PcmTrim(L, H, top_db)


def _run_trim(g, trim, x, frames, out_plane=None, in_off=0, out_off=0):
    """vsyn_pcm_trim_device over x (S, C, plane) float32 with frames [S]: dict(out (S, out_plane), NaN where nothing was written;
    n [S]; bounds (S, 2); ref [S]; ms (S, stride), NaN where nothing was written)."""
    import torch
    S, Cn, plane = x.shape
    out_plane = plane if out_plane is None else out_plane
    buf = torch.zeros(x.size + 8, dtype=torch.float32, device="cuda")
    buf[in_off:in_off + x.size].copy_(torch.from_numpy(np.ascontiguousarray(x).ravel()))
    d_frames = torch.from_numpy(np.asarray(frames, np.int64).astype(np.uint32).view(np.int32)).cuda()
    d_out = torch.full((S * out_plane + 8,), float("nan"), dtype=torch.float32, device="cuda")
    stride = int(g.lib.vsyn_pcm_trim_num_frames(C.byref(trim), min(plane, out_plane))) + 3
    d_ms = torch.full((S, stride), float("nan"), dtype=torch.float64, device="cuda")
    d_ref = torch.full((S,), -7.0, dtype=torch.float64, device="cuda")
    d_bounds = torch.full((S, 2), -1, dtype=torch.int32, device="cuda")
    d_n = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    g.pcm_trim_device(trim, buf.data_ptr() + 4 * in_off, plane, Cn, S, d_frames.data_ptr(), d_out.data_ptr() + 4 * out_off, out_plane,
                      d_n.data_ptr(), d_bounds.data_ptr(), d_ref.data_ptr(), d_ms.data_ptr(), stride, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    flat = d_out.cpu().numpy()
    assert np.isnan(flat[:out_off]).all() and np.isnan(flat[out_off + S * out_plane:]).all()
    return dict(out=flat[out_off:out_off + S * out_plane].reshape(S, out_plane), n=d_n.cpu().numpy().view(np.uint32),
                bounds=d_bounds.cpu().numpy().view(np.uint32), ref=d_ref.cpu().numpy(), ms=d_ms.cpu().numpy())


def _batch(segs, odd):
    """(S, C, plane) from a list of (C, T) arrays: plane a multiple of 4 above the longest (odd: 3 more), zeros past each T."""
    t_max = max(s.shape[1] for s in segs)
    plane = (t_max + 4) // 4 * 4 + (3 if odd else 0)
    x = np.zeros((len(segs), segs[0].shape[0], plane), np.float32)
    for i, s in enumerate(segs):
        x[i, :, :s.shape[1]] = s
    return x, [s.shape[1] for s in segs]


def _check_against_model(g, trim, segs, variant, what):
    """One launch over segs against the model, value by value; returns the worst |d ms| / bound."""
    odd, in_off, out_off = variant
    L, H, top_db = trim.frame_length, trim.hop_length, trim.top_db
    x, frames = _batch(segs, odd)
    out_plane = x.shape[2] + 5
    r = _run_trim(g, trim, x, frames, out_plane, in_off, out_off)
    y, _ = _run_stage(g, _cond(), x, frames, out_plane, in_off, out_off)  # the stage's own downmix
    worst = 0.0
    for gi, T in enumerate(frames):
        w = what + (gi, T)
        mono = y[gi, :T]
        assert np.array_equal(_bits(mono), _bits(tm.downmix(segs[gi]))) if T else True, w
        m = tm.trim(mono, top_db, L, H)
        assert m["margin"] > tm.band(L), (w, m["margin"])  # never skipped: an input inside the band is to be replaced
        F = m["ms"].shape[0]
        ms = r["ms"][gi]
        assert np.isnan(ms[F:]).all() and not np.isnan(ms[:F]).any(), w
        bound = (L + 1) * 2.0 ** -53 * m["ms"]
        d = np.abs(ms[:F] - m["ms"])
        assert (d <= bound).all(), (w, float((d / np.maximum(bound, 1e-300)).max()))
        if F and (bound > 0).any():
            worst = max(worst, float((d[bound > 0] / bound[bound > 0]).max()))
        R = max(float(ms[:F].max()) if F else 0.0, tm.AMIN_SQ)
        assert r["ref"][gi] == R, (w, r["ref"][gi], R)
        assert tuple(int(v) for v in r["bounds"][gi]) == (m["start"], m["end"]), (w, r["bounds"][gi], m["start"], m["end"], m["margin"])
        n = m["end"] - m["start"]
        assert int(r["n"][gi]) == n, w
        assert np.array_equal(_bits(r["out"][gi, :n]), _bits(mono[m["start"]:m["end"]])), w
        assert np.isnan(r["out"][gi, n:]).all(), w  # nothing past out_frames
    return worst


@pytest.mark.parametrize("L,H", tc.LH)
def test_stage_alone_against_the_model(synth, L, H):
    """C = 1 .. 3, the ten lengths and the nine signals of tests/trim_cases.py per (L, H): one segment per (C, T, signal), the short
    lengths in one launch and 4097 / 100003 in another. The five stride / offset variants of the conditioning stage's test are a
    ROTATION over the 42 launches, not a product: each (C, L, H, T, signal) meets one variant, every variant meets every C and
    every (L, H); every variant on one set of segments, bit for bit, is test_exact_properties. The output stride is the input's + 5.
    Measured on the MI355X, worst |d ms| / bound: (2048, 512) 0.0018, (400, 160) 0.0078, (64, 16) 0.046, (7, 3) 0.44, (1, 1) 0,
    (16, 100) 0.14, (8192, 2048) 0.0009."""
    trim = _trim(tc.TOP_DB, L, H)
    worst, k = 0.0, tc.LH.index((L, H))
    for Cn in tc.CHANNELS:
        cs = tc.cases(Cn, L, H)
        small = [x for T, _, x in cs if T < 4097 or T == L or T == L // 2]
        big = [x for T, _, x in cs if not (T < 4097 or T == L or T == L // 2)]
        assert len(small) + len(big) == 10 * len(tc.SIGNALS)
        for part in (small, big):
            worst = max(worst, _check_against_model(synth, trim, part, VARIANTS[k % len(VARIANTS)], (Cn, L, H, k % len(VARIANTS))))
            k += 1
    print("stage alone (L %d, H %d): worst |d ms| / bound %.4f" % (L, H, worst))


def _same(a, b):
    return (np.array_equal(a["bounds"], b["bounds"]) and np.array_equal(a["n"], b["n"]) and np.array_equal(a["ref"].view(np.uint64), b["ref"].view(np.uint64))
            and np.array_equal(a["ms"].view(np.uint64), b["ms"].view(np.uint64)) and np.array_equal(_bits(a["out"]), _bits(b["out"])))


def test_exact_properties(synth):
    """No tolerance: a segment gives the same bounds, ms bits and plane alone, in any slot of a batch and at any alignment; two runs
    give the same bits; 2^k x gives the same bounds (and, above amin, ms scaled exactly)."""
    for (L, H), Cn in (((400, 160), 1), ((2048, 512), 2), ((7, 3), 3), ((16, 100), 2)):
        trim = _trim(tc.TOP_DB, L, H)
        segs = [x for T, kind, x in tc.cases(Cn, L, H) if T in (4097, L, H + 1) and kind in ("mid", "edge", "last_hop", "one_sample")]
        x, frames = _batch(segs, False)
        base = _run_trim(synth, trim, x, frames)
        assert _same(base, _run_trim(synth, trim, x, frames))
        i = len(frames) - 2
        alone = _run_trim(synth, trim, x[i:i + 1], frames[i:i + 1])
        order = [i, 0, len(frames) - 1, 1]
        mixed = _run_trim(synth, trim, x[order], [frames[j] for j in order])
        for a, idx in ((alone, [i]), (mixed, order)):
            for j, src in enumerate(idx):
                assert np.array_equal(a["bounds"][j], base["bounds"][src]) and a["n"][j] == base["n"][src], (L, H, src)
                assert np.array_equal(a["ms"][j].view(np.uint64), base["ms"][src].view(np.uint64)), (L, H, src)
                assert np.array_equal(_bits(a["out"][j]), _bits(base["out"][src])) and a["ref"][j] == base["ref"][src], (L, H, src)
        odd = np.zeros((x.shape[0], Cn, x.shape[2] + 3), np.float32)
        odd[:, :, :x.shape[2]] = x
        o = _run_trim(synth, trim, odd, frames, x.shape[2])
        assert _same(o, base), (L, H, "odd stride")
        for off in (1, 2, 3):
            assert _same(_run_trim(synth, trim, x, frames, None, off, (off + 1) & 3), base), (L, H, off)
    # 2^k x: noise at 0.2 between noise at 2e-3, so that every frame stays above amin at every scale and the sums scale exactly
    rng = np.random.default_rng(12)
    for (L, H), Cn in (((400, 160), 1), ((2048, 512), 3), ((7, 3), 2)):
        trim = _trim(30.0, L, H)
        seg = (rng.standard_normal((Cn, 4097)) * 2e-3).astype(np.float32)
        seg[:, 1300:2900] = (rng.standard_normal((Cn, 1600)) * 0.2).astype(np.float32)
        x, frames = _batch([seg], False)
        base = _run_trim(synth, trim, x, frames)
        F = tm.num_frames(4097, L, H)
        assert 0 < base["bounds"][0, 0] < base["bounds"][0, 1] < 4097 and np.nanmin(base["ms"][0]) > 64 * tm.AMIN_SQ
        for k in (3, -3):
            sc = _run_trim(synth, trim, x * np.float32(2.0 ** k), frames)
            assert np.array_equal(sc["bounds"], base["bounds"]) and np.array_equal(sc["n"], base["n"]), (L, H, k)
            assert np.array_equal(sc["ms"][0, :F], base["ms"][0, :F] * 4.0 ** k) and sc["ref"][0] == base["ref"][0] * 4.0 ** k, (L, H, k)
            assert np.array_equal(_bits(sc["out"]), _bits(base["out"] * np.float32(2.0 ** k)))


def test_a_tiny_top_db_keeps_the_loudest_frame(synth):
    """top_db so small that k rounds to 1 and R * k to R: the loudest frame alone is kept (E >= R), as in the model; never (0, 0)."""
    for top_db in (1e-300, 1e-17, 4e-16):
        trim = _trim(top_db, 400, 160)
        segs = [tc.segment(i, "mid", 2, T, 400, 160) for i, T in enumerate((4097, 9000))]
        x, frames = _batch(segs, False)
        r = _run_trim(synth, trim, x, frames)
        for gi, T in enumerate(frames):
            m = tm.trim(tm.downmix(segs[gi]), top_db, 400, 160)
            assert tuple(int(v) for v in r["bounds"][gi]) == (m["start"], m["end"]) and 0 < r["n"][gi] <= 160, (top_db, gi, r["bounds"][gi])


def test_a_segment_that_is_not_finite_is_refused_alone(synth):
    """An Inf or a NaN, in the loud part, in a frame that would be trimmed, and (H > L) where no frame covers it: that segment gets
    (0, 0), out_frames 0 and a ref that is not finite; its neighbours' results are unchanged bit for bit."""
    for (L, H), Cn in (((400, 160), 2), ((16, 100), 1), ((2048, 2048), 3)):
        trim = _trim(tc.TOP_DB, L, H)
        segs = [tc.segment(i, "mid", Cn, T, L, H) for i, T in enumerate((4097, 20011, 4097, 9000))]
        x, frames = _batch(segs, False)
        want = _run_trim(synth, trim, x, frames)
        assert (want["bounds"][:, 0] > 0).all() and np.isfinite(want["ref"]).all()
        spots = [("loud", 20011 // 2), ("trimmed", 5), ("tail", 20010)]
        if H > L:
            spots.append(("uncovered", 3 * H + L))  # behind frame 3's last sample, in front of frame 4's first
        for value in (np.inf, -np.inf, np.nan, -np.nan):
            for name, t in spots:
                bad = x.copy()
                bad[1, Cn - 1, t] = value
                got = _run_trim(synth, trim, bad, frames)
                w = (L, H, value, name)
                assert not np.isfinite(got["ref"][1]) and tuple(got["bounds"][1]) == (0, 0) and got["n"][1] == 0, w
                assert np.isnan(got["out"][1]).all(), w
                for gi in (0, 2, 3):
                    assert np.array_equal(got["bounds"][gi], want["bounds"][gi]) and got["ref"][gi] == want["ref"][gi], w
                    assert np.array_equal(_bits(got["out"][gi]), _bits(want["out"][gi])), w
                    assert np.array_equal(got["ms"][gi].view(np.uint64), want["ms"][gi].view(np.uint64)), w


BAD_SPECS = [(0, 512, 60.0), (8193, 512, 60.0), (2048, 0, 60.0), (2048, 512, 0.0), (2048, 512, -1.0), (2048, 512, 200.5),
             (2048, 512, float("nan")), (2048, 512, float("inf"))]


def test_bad_arguments_at_every_new_entry_point(synth, mods, blobs):
    """VSYN_ERR_INVALID before anything runs, nothing written."""
    import torch
    from parseoggvorbis_amd import _corpus
    from parseoggvorbis_amd.binding import PcmTrim, Status, Synth, VsynError
    from tests.workloads import fixture_like_spec, synth_batch
    pcm, spectral = mods
    for spec in BAD_SPECS:
        with pytest.raises(VsynError) as ei:
            _run_bad_device(synth, PcmTrim(*spec))
        assert ei.value.code == 1, str(ei.value)
    t = torch.zeros(256, dtype=torch.float32, device="cuda")
    f = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(VsynError) as ei:  # channels = 0
        synth.pcm_trim_device(_trim(), t.data_ptr(), 64, 0, 1, f.data_ptr(), t.data_ptr(), 64, f.data_ptr(), f.data_ptr())
    assert ei.value.code == 1
    # the host entries, on a handle with a submit behind it
    spec = fixture_like_spec(2)
    b = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=31)
    S = len(b["segments"])
    g = Synth(spec, device=0, max_streams=4)
    try:
        assert g.submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"], flags=4)["rc"] == 0
        s = spectral.spectral_spec(kind="log_mel", n_fft=400, hop_length=160, n_mels=40)
        rates = np.full(S, 44100, np.uint32)
        for bad in BAD_SPECS:
            tr = PcmTrim(*bad)
            frames = np.full(S, 77, np.uint64)
            bounds = np.full((S, 2), 77, np.uint32)
            refs = np.full(S, 77.0)
            peaks = np.full(S, 77.0, np.float32)
            out = np.full((S, 4096), 77.0, np.float32)
            err = C.c_char_p()
            rc = g.lib.vsyn_pcm_trim_host(g.h, C.byref(tr), None, S, None, 0, 2, out.ctypes.data, 4096, frames.ctypes.data, bounds.ctypes.data,
                                          peaks.ctypes.data, refs.ctypes.data, C.byref(err))
            assert rc == 1 and err.value, bad
            assert (frames == 77).all() and (bounds == 77).all() and (refs == 77).all() and (peaks == 77).all() and (out == 77).all()
            seg_rows = np.full(S, 77, np.uint64)
            rows = np.full((64, 40), 77.0, np.float32)
            rc = g.lib.vsyn_pcm_trim_spectral_host(g.h, C.byref(tr), None, C.byref(s), None, S, rates.ctypes.data, 0, rows.ctypes.data, 64,
                                                   seg_rows.ctypes.data, bounds.ctypes.data, peaks.ctypes.data, refs.ctypes.data,
                                                   C.byref(Status()), C.byref(err))
            assert rc == 1 and err.value, bad
            assert (seg_rows == 77).all() and (bounds == 77).all() and (refs == 77).all() and (peaks == 77).all() and (rows == 77).all()
    finally:
        g.close()
    # the corpus entries refuse the call
    lib = pcm._load()
    n = len(blobs)
    for bad in BAD_SPECS:
        tr = PcmTrim(*bad)
        frames, chans, rts, bounds = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, 2), np.uint64)
        with pytest.raises(pcm.PcmError, match="invalid trim spec"):
            _corpus.run(lib, lib.ogg_vorbis_pcm_corpus_trim, blobs, (4, 2, 64, 0, 0, 2, None, C.byref(tr)), (frames, chans, rts, bounds),
                        lambda i, p: None, pcm.PcmError, "raise", "pcm")
        counts = np.zeros(n, np.uint64)
        with pytest.raises(spectral.SpectralError, match="invalid trim spec"):
            _corpus.run(lib, lib.ogg_vorbis_spectral_corpus_trim, blobs, (4, 2, 64, 0, C.byref(s), 0, None, None, C.byref(tr)), (counts, bounds),
                        lambda i, p: None, spectral.SpectralError, "raise", "spectral")


def _run_bad_device(g, trim):
    """vsyn_pcm_trim_device with a spec it must refuse: every output keeps its fill."""
    import torch
    t = torch.full((256,), 5.0, dtype=torch.float32, device="cuda")
    f = torch.full((8,), 64, dtype=torch.int32, device="cuda")
    o = torch.full((8,), 9, dtype=torch.int32, device="cuda")
    try:
        g.pcm_trim_device(trim, t.data_ptr(), 64, 2, 1, f.data_ptr(), t.data_ptr() + 512, 64, o.data_ptr(), o.data_ptr() + 8)
    finally:
        torch.cuda.synchronize()
        assert (t.cpu().numpy() == 5.0).all() and (o.cpu().numpy() == 9).all()


def test_stage_off_means_off(mods, blobs, pcm_by_rate):
    """trim_db=None: get_pcm_batch and get_spectral_batch give today's bits, the corpus statistics show no extra work, and a NULL
    vsyn_pcm_trim at the host and corpus entries equals the entries without the stage."""
    from parseoggvorbis_amd import _corpus
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec, synth_batch
    pcm, spectral = mods
    lib = pcm._load()
    n = len(blobs)
    for sr in (None, 16000):
        st0, st1, idx = [], [], []
        got = pcm.get_pcm_batch(blobs, sr=sr, trim_db=None, trim_frame_length=400, trim_hop_length=160, trim_index=idx, stats=st1, feeders=1)
        ref = pcm.get_pcm_batch(blobs, sr=sr, stats=st0, feeders=1)  # (one feeder: the submit count does not depend on timing)
        for name, (y, r), (y0, r0) in zip(FILES, got, ref):
            want = pcm_by_rate[sr][name]
            assert r == r0 and y.shape == want.shape and np.array_equal(_bits(y), _bits(want)) and np.array_equal(_bits(y), _bits(y0)), (name, sr)
        assert idx == [None] * n  # the stage is off: there are no bounds
        assert st0[5:] == st1[5:]  # submits, audio packets, frames: the same work
        for kw in (dict(mono=True), dict(mono=True, peak_normalize=True, preemphasis=A)):
            a = pcm.get_pcm_batch(blobs, sr=sr, **kw)
            b = pcm.get_pcm_batch(blobs, sr=sr, trim_db=None, **kw)
            frames, chans, rts, bounds = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.ones((n, 2), np.uint64)
            cond = pcm.cond_spec(kw.get("peak_normalize", False), kw.get("preemphasis"))
            c = _corpus.run(lib, lib.ogg_vorbis_pcm_corpus_trim, blobs, (4, 2, 64, 0, sr or 0, 2, C.byref(cond), None), (frames, chans, rts, bounds),
                            lambda i, p: _corpus.copy_into(np.zeros(int(frames[i]), np.float32), p), pcm.PcmError, "raise", "pcm")
            assert not bounds.any()
            for (p, _), (q, _), r in zip(a, b, c):
                assert np.array_equal(_bits(p), _bits(q)) and p.shape == r.shape and np.array_equal(_bits(p), _bits(r))
        for kw in (E2E[0], E2E[1]):
            st0, st1, idx = [], [], []
            a = spectral.get_spectral_batch(blobs, sr=sr, stats=st0, feeders=1, **kw)
            b = spectral.get_spectral_batch(blobs, sr=sr, trim_db=None, trim_index=idx, stats=st1, feeders=1, **kw)
            assert idx == [None] * n and st0[5:] == st1[5:]
            s = spectral.spectral_spec(**kw)
            counts, bounds = np.zeros(n, np.uint64), np.ones((n, 2), np.uint64)
            dim = spectral.spec_dim(s)
            c = _corpus.run(lib, lib.ogg_vorbis_spectral_corpus_trim, blobs, (4, 2, 64, 0, C.byref(s), sr or 0, None, None, None), (counts, bounds),
                            lambda i, p: _corpus.copy_into(np.zeros((int(counts[i]), dim), np.float32), p), spectral.SpectralError, "raise",
                            "spectral")
            for p, q, r in zip(a, b, c):
                assert np.array_equal(_bits(p), _bits(q)) and p.shape == r.shape and np.array_equal(_bits(p), _bits(r))
    # the host entries with a NULL trim
    spec = fixture_like_spec(2)
    bt = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=11)
    S = len(bt["segments"])
    g = Synth(spec, device=0, max_streams=4)
    try:
        assert g.submit_host(bt["packets"], bt["segments"], bt["ys"], bt["residue"], bt["plane_stride"], flags=4)["rc"] == 0
        s = spectral.spectral_spec(kind="log_mel", n_fft=400, hop_length=160, n_mels=40)
        for cond in (_cond(), _cond(True, A)):
            for fmt in (2, 1):
                out, frames, peaks = g.pcm_condition_host(cond, S, fmt=fmt)
                off = g.pcm_trim_host(None, cond, S, fmt=fmt)
                assert np.array_equal(off["pcm"].view(np.uint8), out.view(np.uint8)) and np.array_equal(off["frames"], frames)
                assert np.array_equal(_bits(off["peaks"]), _bits(peaks)) and not off["bounds"].any() and not off["refs"].any()
            want = g.pcm_cond_spectral_host(cond, s, None, [44100] * S)
            off = g.pcm_trim_spectral_host(None, cond, s, None, [44100] * S)
            assert np.array_equal(_bits(off["rows"]), _bits(want["rows"])) and np.array_equal(off["seg_rows"], want["seg_rows"])
            assert np.array_equal(_bits(off["peaks"]), _bits(want["peaks"])) and not off["bounds"].any()
    finally:
        g.close()


@pytest.mark.parametrize("sr", [None, 16000])
def test_trimmed_pcm_end_to_end(mods, blobs, synth, sr):
    """get_pcm_batch(mono=True, trim_db=d, ...) on every fixture equals get_pcm_batch(mono=True) sliced at the model's bounds (the
    model on that device plane), bit for bit, and trim_index equals those bounds; with peak_normalize and preemphasis it equals the
    conditioning stage alone over the sliced plane as 1-channel input; int16 is the existing conversion of those planes."""
    pcm, _ = mods
    planes = pcm.get_pcm_batch(blobs, sr=sr, mono=True)
    smallest = {}
    for d, L, H in E2E_TRIM:
        kw = dict(sr=sr, mono=True, trim_db=d, trim_frame_length=L, trim_hop_length=H)
        idx, idx2 = [], []
        got = pcm.get_pcm_batch(blobs, trim_index=idx, **kw)
        got16 = pcm.get_pcm_batch(blobs, dtype="int16", **kw)
        cnd = pcm.get_pcm_batch(blobs, peak_normalize=True, preemphasis=A, trim_index=idx2, **kw)
        cnd16 = pcm.get_pcm_batch(blobs, dtype="int16", peak_normalize=True, preemphasis=A, **kw)
        assert idx == idx2
        for i, (name, data) in enumerate(zip(FILES, blobs)):
            y = planes[i][0]
            m = tm.trim(y, d, L, H)
            smallest[(d, L, H)] = min(smallest.get((d, L, H), np.inf), m["margin"])
            assert m["margin"] > tm.band(L), (name, d, L, H, m["margin"])
            w = (name, sr, d, L, H, m["start"], m["end"])
            cut = y[m["start"]:m["end"]]
            assert idx[i] == (m["start"], m["end"]), (w, idx[i])
            assert got[i][1] == (sr or _rate(data)) and got[i][0].dtype == np.float32
            assert got[i][0].shape == cut.shape and np.array_equal(_bits(got[i][0]), _bits(cut)), w
            assert np.array_equal(got16[i][0], _s16(cut)), w
            want, _ = _stage_on_file(synth, _cond(True, A), cut[None, :])
            assert cnd[i][0].shape == want.shape and np.array_equal(_bits(cnd[i][0]), _bits(want)), w
            assert np.array_equal(cnd16[i][0], _s16(want)), w
    print("trim end to end (sr %s): smallest margin per parameter set" % sr, {k: float("%.3g" % v) for k, v in smallest.items()})


def test_trimmed_spectral_rows_equal_the_model(mods, blobs):
    """get_spectral_batch(trim_db=...) against tests/spectral_model.py on the device's own trimmed plane under GATE, unchanged; with
    delta=2, normalize="mean_var" under the post tests' composed gate, where a file trimmed below delta_width frames fails alone
    (most fixtures under (20, 64, 16)); with peak_normalize and preemphasis on top of the trim as well."""
    pcm, spectral = mods
    worst = {}
    for sr, (d, L, H), kws in ((None, E2E_TRIM[0], E2E), (16000, E2E_TRIM[1], E2E[:1]), (None, E2E_TRIM[2], E2E[:1])):
        tk = dict(trim_db=d, trim_frame_length=L, trim_hop_length=H)
        for cond in (dict(), dict(peak_normalize=True, preemphasis=A)):
            idx, idx2 = [], []
            planes = pcm.get_pcm_batch(blobs, sr=sr, mono=True, trim_index=idx, **tk, **cond)
            for kw in kws:
                res = spectral.get_spectral_batch(blobs, sr=sr, trim_index=idx2, **tk, **cond, **kw)
                assert idx2 == idx
                for name, (y, r), got in zip(FILES, planes, res):
                    e = assert_matches(got, y[None, :], r, kw, (name, sr, d, L, H, kw["kind"]))
                    worst[kw["kind"]] = max(worst.get(kw["kind"], 0.0), e / GATE[kw["kind"]])
            shim = types.SimpleNamespace(get_spectral_batch=functools.partial(spectral.get_spectral_batch, **tk, **cond),
                                         SpectralError=spectral.SpectralError)
            as_pcm = {sr: {name: y[None, :] for name, (y, _) in zip(FILES, planes)}}
            n, w = _compare_batch(shim, as_pcm, E2E[0], 2, 9, "mean_var", sr)
            short = sum(1 for y, _ in planes if 0 < 1 + y.shape[0] // 160 < 9)
            assert n > 0 and n + short <= len(FILES)
            if (d, L, H) == E2E_TRIM[2]:
                assert short > 0  # the case is there: files trimmed below the delta width, failing alone
            worst["post/%s/%d" % (sr, L)] = max(worst.get("post/%s/%d" % (sr, L), 0.0), w)
    print("trimmed rows, worst |d| / gate:", {k: round(v, 4) for k, v in sorted(worst.items())})


def test_host_entries_leave_the_pcm_and_the_next_submit_alone_and_chain(mods, synth):
    """vsyn_pcm_trim_host and vsyn_pcm_trim_spectral_host between two submits: vsyn_pcm_fetch_host and the next submit are
    bit-identical to a handle that made no such call. The full chain in one call (resample, trim, condition, STFT / mel, post)
    equals vsyn_resample_device -> vsyn_pcm_trim_device -> vsyn_pcm_condition_device (1 channel) -> vsyn_spectral_device ->
    vsyn_spectral_post_device run one by one on the fetched PCM, on planes of another stride; the PCM of vsyn_pcm_trim_host, F32 and
    S16, equals that run's conditioned plane. Three segments at 16000 (ratio 1), 0 (skipped) and 8000 Hz (resampled 1:2)."""
    import torch
    from parseoggvorbis_amd.binding import Synth, VSYN_PCM_F32, VSYN_PCM_S16
    from tests.workloads import fixture_like_spec, synth_batch
    _, spectral = mods
    spec = fixture_like_spec(2)
    b1 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=21)
    b2 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=22)
    S, Cn, rates, out_rate = len(b1["segments"]), 2, [16000, 0, 8000], 16000
    cond = _cond(True, A)
    trim = _trim(3.0, 64, 16)
    s = spectral.spectral_spec(kind="mel_db", n_fft=64, hop_length=32, n_mels=8)
    dim = spectral.spec_dim(s)
    post, dout, _ = spectral.post_spec(dim, delta=1, delta_width=3, normalize="mean_var")
    outs = []
    for with_trim in (False, True):
        g = Synth(spec, device=0, max_streams=4)
        try:
            assert g.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"], flags=4)["rc"] == 0
            f1, fr = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
            if with_trim:
                host = g.pcm_trim_spectral_host(trim, cond, s, post, rates, out_rate)
                h32 = g.pcm_trim_host(trim, cond, S, rates, out_rate)
                h16 = g.pcm_trim_host(trim, cond, S, rates, out_rate, fmt=VSYN_PCM_S16)
                plain = g.pcm_trim_host(trim, None, S, rates, out_rate)
            f1b, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
            assert np.array_equal(f1, f1b)
            r2 = g.submit_host(b2["packets"], b2["segments"], b2["ys"], b2["residue"], b2["plane_stride"])
            assert r2["rc"] == 0
            outs.append((f1, r2["pcm"], r2["emit_len"]))
        finally:
            g.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    assert host["rc"] == 0
    T = [int(t) * out_rate // r if r else 0 for t, r in zip(fr, rates)]
    t_max = max(T)
    plane = t_max + 5
    in_plane = plane // 2
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
    d_tr = torch.full((S * plane,), float("nan"), dtype=torch.float32, device="cuda")
    d_trf = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    d_bd = torch.full((S, 2), -1, dtype=torch.int32, device="cuda")
    d_ref = torch.full((S,), -1.0, dtype=torch.float64, device="cuda")
    synth.pcm_trim_device(trim, d_rs.data_ptr(), plane, Cn, S, d_rsf.data_ptr(), d_tr.data_ptr(), plane, d_trf.data_ptr(), d_bd.data_ptr(),
                          d_ref.data_ptr(), None, 0, st)
    d_cd = torch.full((S * plane,), float("nan"), dtype=torch.float32, device="cuda")
    d_pk = torch.full((S,), float("nan"), dtype=torch.float32, device="cuda")
    synth.pcm_condition_device(cond, d_tr.data_ptr(), plane, 1, S, d_trf.data_ptr(), d_cd.data_ptr(), plane, d_pk.data_ptr(), st)
    torch.cuda.synchronize()
    bd = d_bd.cpu().numpy()
    n = [int(e - a) for a, e in bd]
    assert list(d_trf.cpu().numpy()) == n and n[1] == 0 and 0 < n[0] <= T[0] and 0 < n[2] <= T[2]
    assert n[0] < T[0] or n[2] < T[2]  # 3 dB under the loudest frame: something is cut
    n_rows = [int(synth.lib.vsyn_spectral_num_frames(C.byref(s), t)) if r else 0 for t, r in zip(n, rates)]
    total = sum(n_rows)
    d_rows = torch.full((total + 2, dim), float("nan"), dtype=torch.float32, device="cuda")
    d_off = torch.full((S + 1,), -1, dtype=torch.int64, device="cuda")
    synth.spectral_device(s, [out_rate if r else 0 for r in rates], d_cd.data_ptr(), plane, 1, d_trf.data_ptr(), d_rows.data_ptr(),
                          d_off.data_ptr(), st)
    d_post = torch.full((total + 2, dout), float("nan"), dtype=torch.float32, device="cuda")
    synth.spectral_post_device(post, dim, n_rows, d_rows.data_ptr(), d_post.data_ptr(), st)
    torch.cuda.synchronize()
    assert list(host["seg_rows"]) == n_rows and min(n_rows[0], n_rows[2]) >= 3
    want_rows = d_post.cpu().numpy()
    assert host["rows"].shape == (total, dout) and np.array_equal(_bits(host["rows"]), _bits(want_rows[:total]))
    pk, refs = d_pk.cpu().numpy(), d_ref.cpu().numpy()
    for r in (host, h32, h16, plain):
        assert np.array_equal(r["bounds"].astype(np.int64), bd.astype(np.int64)) and np.array_equal(r["refs"], refs)
    assert np.array_equal(_bits(host["peaks"]), _bits(pk)) and np.array_equal(_bits(h32["peaks"]), _bits(pk)) and not plain["peaks"].any()
    cd = d_cd.cpu().numpy().reshape(S, plane)
    tr = d_tr.cpu().numpy().reshape(S, plane)
    assert h32["pcm"].shape == (S, t_max) and list(h32["frames"]) == n and list(h16["frames"]) == n and list(plain["frames"]) == n
    for gi in range(S):
        assert np.isnan(tr[gi, n[gi]:]).all() and np.isnan(cd[gi, n[gi]:]).all()
        assert np.array_equal(_bits(h32["pcm"][gi, :n[gi]]), _bits(cd[gi, :n[gi]])) and not h32["pcm"][gi, n[gi]:].any(), gi
        assert np.array_equal(h16["pcm"][gi, :n[gi]], _s16(cd[gi, :n[gi]])) and not h16["pcm"][gi, n[gi]:].any(), gi
        assert np.array_equal(_bits(plain["pcm"][gi, :n[gi]]), _bits(tr[gi, :n[gi]])) and not plain["pcm"][gi, n[gi]:].any(), gi
