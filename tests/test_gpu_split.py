"""PCM splitting on the GPU (vsyn_pcm_split_device, vsyn_pcm_split_host, vsyn_pcm_split_intervals_host, vsyn_pcm_split_spectral_host,
ogg_vorbis_pcm_corpus_split, ogg_vorbis_spectral_corpus_split, ogg_vorbis_intervals_corpus, get_pcm_batch(split_db=, ...),
get_spectral_batch(split_db=, ...), get_intervals_batch) against the float64 model of tests/split_model.py.

Gates of the stage alone:
    ms[f]         the trim stage's: |d| <= (L + 1) * 2^-53 * ms[f]; and the trim entry's ms array bit for bit.
    R             max(ms) of the device's own d_ms (or 1e-10), exactly.
    intervals     the model's, count and values, on inputs whose model margin is above (2L + 3) * 2^-53 (asserted here and, without a
                  GPU, in tests/test_split_cpu.py).
    plane         the concatenation of the stage's own downmix (the conditioning stage with options = 0) sliced at the intervals, bit
                  for bit; nothing behind out_frames.
End to end the truth is the model on the device's own mono plane; for the conditioned signal the gates of tests/test_gpu_condition.py
and for the rows GATE of tests/test_gpu_spectral.py and the post tests' composed gate, unchanged.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from tests import condition_model as cm
from tests import split_cases as sc
from tests import split_model as sm
from tests import trim_model as tm
from tests.test_gpu_condition import A, U, _bits, _cond, _run_stage, _s16, blobs, mods, pcm_by_rate, synth  # noqa: F401
from tests.test_gpu_spectral import FILES, GATE, _rate, assert_matches
from tests.test_gpu_spectral_post import E2E, _compare_batch
from tests.test_gpu_trim import BAD_SPECS, E2E_TRIM, VARIANTS, _batch, _run_trim, _trim

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF


def _run_split(g, split, x, frames, out_plane=None, in_off=0, out_off=0, stride_extra=3):
    """vsyn_pcm_split_device over x (S, C, plane) float32 with frames [S]: dict(out (S, out_plane), NaN where nothing was written;
    n [S]; counts [S]; iv: a list of (count, 2) int64 arrays; ref [S]; ms (S, stride), NaN where nothing was written). Asserts that
    no interval word behind a segment's count was written."""
    import torch
    S, Cn, plane = x.shape
    out_plane = plane if out_plane is None else out_plane
    buf = torch.zeros(x.size + 8, dtype=torch.float32, device="cuda")
    buf[in_off:in_off + x.size].copy_(torch.from_numpy(np.ascontiguousarray(x).ravel()))
    d_frames = torch.from_numpy(np.asarray(frames, np.int64).astype(np.uint32).view(np.int32)).cuda()
    d_out = torch.full((S * out_plane + 8,), float("nan"), dtype=torch.float32, device="cuda")
    stride = int(g.lib.vsyn_pcm_trim_num_frames(C.byref(split), min(plane, out_plane))) + 3
    ivs = int(g.lib.vsyn_pcm_split_max_intervals(C.byref(split), min(plane, out_plane))) + stride_extra
    d_ms = torch.full((S, stride), float("nan"), dtype=torch.float64, device="cuda")
    d_ref = torch.full((S,), -7.0, dtype=torch.float64, device="cuda")
    d_iv = torch.from_numpy(np.full((S, ivs, 2), SENTINEL, np.uint32).view(np.int32)).cuda()
    d_cnt = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    d_n = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    g.pcm_split_device(split, buf.data_ptr() + 4 * in_off, plane, Cn, S, d_frames.data_ptr(), d_out.data_ptr() + 4 * out_off, out_plane,
                       d_n.data_ptr(), d_cnt.data_ptr(), d_iv.data_ptr(), ivs, d_ref.data_ptr(), d_ms.data_ptr(), stride,
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    flat = d_out.cpu().numpy()
    assert np.isnan(flat[:out_off]).all() and np.isnan(flat[out_off + S * out_plane:]).all()
    counts = d_cnt.cpu().numpy().view(np.uint32)
    iv = d_iv.cpu().numpy().view(np.uint32)
    assert (counts <= ivs - stride_extra).all()
    for gi in range(S):
        assert (iv[gi, int(counts[gi]):] == SENTINEL).all(), gi
    return dict(out=flat[out_off:out_off + S * out_plane].reshape(S, out_plane), n=d_n.cpu().numpy().view(np.uint32), counts=counts,
                iv=[iv[gi, :int(counts[gi])].astype(np.int64) for gi in range(S)], ref=d_ref.cpu().numpy(), ms=d_ms.cpu().numpy())


def _check_against_model(g, split, segs, variant, what):
    """One launch over segs against the model, value by value; returns (worst |d ms| / bound, most intervals)."""
    odd, in_off, out_off = variant
    L, H, top_db = split.frame_length, split.hop_length, split.top_db
    x, frames = _batch(segs, odd)
    out_plane = x.shape[2] + 5
    r = _run_split(g, split, x, frames, out_plane, in_off, out_off)
    y, _ = _run_stage(g, _cond(), x, frames, out_plane, in_off, out_off)  # the stage's own downmix
    worst, most = 0.0, 0
    for gi, T in enumerate(frames):
        w = what + (gi, T)
        mono = y[gi, :T]
        assert np.array_equal(_bits(mono), _bits(tm.downmix(segs[gi]))) if T else True, w
        m = sm.split(mono, top_db, L, H)
        assert m["margin"] > sm.band(L), (w, m["margin"])  # never skipped: an input inside the band is to be replaced
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
        assert int(r["counts"][gi]) == len(m["intervals"]), (w, int(r["counts"][gi]), len(m["intervals"]), m["margin"])
        assert np.array_equal(r["iv"][gi], m["intervals"]), w
        joined = np.concatenate([mono[a:b] for a, b in r["iv"][gi]]) if len(r["iv"][gi]) else mono[:0]
        n = joined.shape[0]
        assert int(r["n"][gi]) == n == m["joined"].shape[0], w
        assert np.array_equal(_bits(r["out"][gi, :n]), _bits(joined)), w
        assert np.isnan(r["out"][gi, n:]).all(), w  # nothing past out_frames
        most = max(most, len(m["intervals"]))
    return worst, most


@pytest.mark.parametrize("L,H", sc.LH)
def test_stage_alone_against_the_model(synth, L, H):
    """C = 1 .. 3, the ten lengths and the twelve signals of tests/split_cases.py per (L, H): one segment per (C, T, signal), the short
    lengths in one launch and 4097 / 100003 in another, the five stride / offset variants of the trim stage's test in rotation. The
    output stride is the input's + 5, the interval stride 3 above the least allowed."""
    split = _trim(sc.TOP_DB, L, H)
    worst, most, k = 0.0, 0, sc.LH.index((L, H))
    for Cn in sc.CHANNELS:
        cs = sc.cases(Cn, L, H)
        small = [x for T, _, x in cs if T < 4097 or T == L or T == L // 2]
        big = [x for T, _, x in cs if not (T < 4097 or T == L or T == L // 2)]
        assert len(small) + len(big) == 10 * len(sc.SIGNALS)
        for part in (small, big):
            w, n = _check_against_model(synth, split, part, VARIANTS[k % len(VARIANTS)], (Cn, L, H, k % len(VARIANTS)))
            worst, most = max(worst, w), max(most, n)
            k += 1
    print("split alone (L %d, H %d): worst |d ms| / bound %.4f, most intervals %d" % (L, H, worst, most))
    if (L, H) == (1, 1):
        assert most > 45000  # the scan's chunk carry, many times over
    if (L, H) == (16, 100):
        assert most == 501


def _same(a, b):
    return (np.array_equal(a["counts"], b["counts"]) and all(np.array_equal(p, q) for p, q in zip(a["iv"], b["iv"])) and np.array_equal(a["n"], b["n"])
            and np.array_equal(a["ref"].view(np.uint64), b["ref"].view(np.uint64)) and np.array_equal(a["ms"].view(np.uint64), b["ms"].view(np.uint64))
            and np.array_equal(_bits(a["out"]), _bits(b["out"])))


def test_exact_properties(synth):
    """No tolerance: a segment gives the same intervals, ms bits and plane alone, as the third of five and at four alignments; two
    runs give the same bits; the first start and the last end are vsyn_pcm_trim_device's (start, end), and the ms array is the
    trim entry's, bit for bit."""
    for (L, H), Cn in (((400, 160), 1), ((2048, 512), 2), ((7, 3), 3), ((16, 100), 2), ((64, 16), 1)):
        split = _trim(sc.TOP_DB, L, H)
        segs = [x for T, kind, x in sc.cases(Cn, L, H) if T in (4097, L, H + 1) and kind in ("mid", "edge", "last_hop", "bursts", "alternate", "last_frame")]
        x, frames = _batch(segs, False)
        base = _run_split(synth, split, x, frames)
        assert _same(base, _run_split(synth, split, x, frames))
        assert max(int(c) for c in base["counts"]) > 1
        tr = _run_trim(synth, split, x, frames)
        assert np.array_equal(tr["ms"].view(np.uint64), base["ms"].view(np.uint64)) and np.array_equal(tr["ref"].view(np.uint64), base["ref"].view(np.uint64))
        for gi in range(len(frames)):
            assert (int(base["iv"][gi][0, 0]), int(base["iv"][gi][-1, 1])) == tuple(int(v) for v in tr["bounds"][gi]), (L, H, gi)
        i = len(frames) - 2
        alone = _run_split(synth, split, x[i:i + 1], frames[i:i + 1])
        order = [0, 1, i, len(frames) - 1, 2]  # the third of five
        mixed = _run_split(synth, split, x[order], [frames[j] for j in order])
        for a, idx in ((alone, [i]), (mixed, order)):
            for j, src in enumerate(idx):
                assert np.array_equal(a["iv"][j], base["iv"][src]) and a["n"][j] == base["n"][src], (L, H, src)
                assert np.array_equal(a["ms"][j].view(np.uint64), base["ms"][src].view(np.uint64)), (L, H, src)
                assert np.array_equal(_bits(a["out"][j]), _bits(base["out"][src])) and a["ref"][j] == base["ref"][src], (L, H, src)
        odd = np.zeros((x.shape[0], Cn, x.shape[2] + 3), np.float32)
        odd[:, :, :x.shape[2]] = x
        assert _same(_run_split(synth, split, odd, frames, x.shape[2]), base), (L, H, "odd stride")
        for off in (1, 2, 3):
            assert _same(_run_split(synth, split, x, frames, None, off, (off + 1) & 3), base), (L, H, off)


def test_a_segment_that_is_not_finite_is_refused_alone(synth):
    """An Inf or a NaN, in a loud part, in a silent part, and (H > L) where no frame covers it: that segment gets no intervals,
    out_frames 0 and a ref that is not finite; its neighbours' results are unchanged bit for bit."""
    for (L, H), Cn in (((400, 160), 2), ((16, 100), 1), ((2048, 2048), 3)):
        split = _trim(sc.TOP_DB, L, H)
        segs = [sc.segment(i, "bursts", Cn, T, L, H) for i, T in enumerate((4097, 20011, 4097))]
        x, frames = _batch(segs, False)
        want = _run_split(synth, split, x, frames)
        assert (want["counts"] >= 1).all() and np.isfinite(want["ref"]).all()
        spots = [("loud", 20011 // 9 + 5), ("silent", 5), ("tail", 20010)]
        if H > L:
            spots.append(("uncovered", 3 * H + L))  # behind frame 3's last sample, in front of frame 4's first
        for value in (np.inf, -np.inf, np.nan):
            for name, t in spots:
                bad = x.copy()
                bad[1, Cn - 1, t] = value
                got = _run_split(synth, split, bad, frames)
                w = (L, H, value, name)
                assert not np.isfinite(got["ref"][1]) and got["counts"][1] == 0 and got["n"][1] == 0, w
                assert np.isnan(got["out"][1]).all(), w
                for gi in (0, 2):
                    assert np.array_equal(got["iv"][gi], want["iv"][gi]) and got["ref"][gi] == want["ref"][gi] and got["n"][gi] == want["n"][gi], w
                    assert np.array_equal(_bits(got["out"][gi]), _bits(want["out"][gi])), w
                    assert np.array_equal(got["ms"][gi].view(np.uint64), want["ms"][gi].view(np.uint64)), w


def test_bad_arguments_at_every_new_entry_point(synth, mods, blobs):
    """VSYN_ERR_INVALID before anything runs, nothing written: a bad spec, channels = 0, an interval stride one below the least."""
    import torch
    from parseoggvorbis_amd import _corpus
    from parseoggvorbis_amd.binding import PcmTrim, Status, Synth, VsynError
    from tests.workloads import fixture_like_spec, synth_batch
    pcm, spectral = mods
    assert synth.lib.vsyn_pcm_split_max_intervals(C.byref(_trim()), 0) == 0
    assert synth.lib.vsyn_pcm_split_max_intervals(C.byref(_trim(60.0, 16, 100)), 100000) == 501
    assert synth.lib.vsyn_pcm_split_max_intervals(C.byref(PcmTrim(0, 512, 60.0)), 100000) == 0

    def device(split, channels=2, ivs=None):
        t = torch.full((256,), 5.0, dtype=torch.float32, device="cuda")
        f = torch.full((8,), 64, dtype=torch.int32, device="cuda")
        o = torch.full((64,), 9, dtype=torch.int32, device="cuda")
        try:
            synth.pcm_split_device(split, t.data_ptr(), 64, channels, 1, f.data_ptr(), t.data_ptr() + 512, 64, o.data_ptr(), o.data_ptr() + 8,
                                   o.data_ptr() + 16, 1 if ivs is None else ivs)
        finally:
            torch.cuda.synchronize()
            assert (t.cpu().numpy() == 5.0).all() and (o.cpu().numpy() == 9).all()
    for bad in BAD_SPECS:
        with pytest.raises(VsynError) as ei:
            device(PcmTrim(*bad))
        assert ei.value.code == 1, str(ei.value)
    for kw in (dict(channels=0), dict(split=_trim(60.0, 1, 1), ivs=31)):  # (L = H = 1, 64 frames: 32 intervals at the most)
        with pytest.raises(VsynError) as ei:
            device(kw.get("split", _trim()), kw.get("channels", 2), kw.get("ivs"))
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
        t_max = int(g.pcm_split_intervals_host(_trim(60.0, 1, 1), S)["frames"].max())
        need = int(g.lib.vsyn_pcm_split_max_intervals(C.byref(_trim(60.0, 1, 1)), t_max))
        assert need == (t_max + 1) // 2 and need > 1
        for tr, ivs in [(PcmTrim(*bad), need) for bad in BAD_SPECS] + [(_trim(60.0, 1, 1), need - 1)]:
            frames = np.full(S, 77, np.uint64)
            counts = np.full(S, 77, np.uint32)
            iv = np.full((S, need, 2), 77, np.uint32)
            refs = np.full(S, 77.0)
            peaks = np.full(S, 77.0, np.float32)
            out = np.full((S, t_max), 77.0, np.float32)
            err = C.c_char_p()
            stride_case = tr.frame_length == 1 and tr.top_db == 60.0
            rc = g.lib.vsyn_pcm_split_host(g.h, C.byref(tr), None, S, None, 0, 2, out.ctypes.data, t_max, frames.ctypes.data, counts.ctypes.data,
                                           iv.ctypes.data, ivs, peaks.ctypes.data, refs.ctypes.data, C.byref(err))
            assert rc == 1 and err.value, (tr.frame_length, ivs)
            assert (counts == 77).all() and (iv == 77).all() and (refs == 77).all() and (out == 77).all()
            assert stride_case or ((frames == 77).all() and (peaks == 77).all())  # (the stride is checked with the frames known)
            frames[:] = 77
            rc = g.lib.vsyn_pcm_split_intervals_host(g.h, C.byref(tr), S, None, 0, frames.ctypes.data, counts.ctypes.data, iv.ctypes.data, ivs,
                                                     refs.ctypes.data, C.byref(err))
            assert rc == 1 and err.value, (tr.frame_length, ivs)
            assert (counts == 77).all() and (iv == 77).all() and (refs == 77).all() and (stride_case or (frames == 77).all())
            seg_rows = np.full(S, 77, np.uint64)
            rows = np.full((64, 40), 77.0, np.float32)
            frames[:] = 77
            rc = g.lib.vsyn_pcm_split_spectral_host(g.h, C.byref(tr), None, C.byref(s), None, S, rates.ctypes.data, 0, rows.ctypes.data, 64,
                                                    seg_rows.ctypes.data, frames.ctypes.data, counts.ctypes.data, iv.ctypes.data, ivs,
                                                    peaks.ctypes.data, refs.ctypes.data, C.byref(Status()), C.byref(err))
            assert rc == 1 and err.value, (tr.frame_length, ivs)
            assert (frames == 77).all() and (counts == 77).all() and (iv == 77).all() and (rows == 77).all()
            assert stride_case or ((seg_rows == 77).all() and (refs == 77).all())
    finally:
        g.close()
    # the corpus entries refuse the call
    lib = pcm._load()
    n = len(blobs)
    for bad in BAD_SPECS:
        tr = PcmTrim(*bad)
        frames, chans, rts, cnt = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
        ib = _corpus.IntervalBuffers(lib, n)
        with pytest.raises(pcm.PcmError, match="invalid split spec"):
            _corpus.run(lib, lib.ogg_vorbis_pcm_corpus_split, blobs, (4, 2, 64, 0, 0, 2, None, C.byref(tr)), (frames, chans, rts, ib.ptrs, ib.counts),
                        lambda i, p: None, pcm.PcmError, "raise", "pcm")
        with pytest.raises(spectral.SpectralError, match="invalid split spec"):
            _corpus.run(lib, lib.ogg_vorbis_spectral_corpus_split, blobs, (4, 2, 64, 0, C.byref(s), 0, None, None, C.byref(tr)),
                        (cnt, frames, ib.ptrs, ib.counts), lambda i, p: None, spectral.SpectralError, "raise", "spectral")
        with pytest.raises(pcm.PcmError, match="invalid split spec"):
            _corpus.run(lib, lib.ogg_vorbis_intervals_corpus, blobs, (4, 2, 64, 0, 0, C.byref(tr)), (cnt, frames, rts), lambda i, p: None,
                        pcm.PcmError, "raise", "intervals")
        assert not any(ib.ptrs) and not ib.counts.any()
    # Python: refused before the library is touched (the CPU tests cover every value; here with the library loaded)
    for kw in (dict(split_db=0), dict(split_db=60.0, trim_db=60.0), dict(split_db=60.0, split_frame_length=8193)):
        with pytest.raises(pcm.PcmError):
            pcm.get_pcm_batch(blobs, mono=True, **kw)
        with pytest.raises(spectral.SpectralError):
            spectral.get_spectral_batch(blobs, **kw)
    with pytest.raises(pcm.PcmError):
        pcm.get_pcm_batch(blobs, split_db=60.0)
    with pytest.raises(pcm.PcmError):
        pcm.get_intervals_batch(blobs, top_db=0)


def test_stage_off_means_off(mods, blobs, pcm_by_rate):
    """split_db=None: get_pcm_batch and get_spectral_batch give today's bits and the corpus statistics show no extra work; a NULL spec
    at the host and corpus entries equals the entries without the stage."""
    from parseoggvorbis_amd import _corpus
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec, synth_batch
    pcm, spectral = mods
    lib = pcm._load()
    n = len(blobs)
    for sr in (None, 16000):
        st0, st1, idx = [], [], []
        got = pcm.get_pcm_batch(blobs, sr=sr, split_db=None, split_frame_length=400, split_hop_length=160, split_index=idx, stats=st1, feeders=1)
        ref = pcm.get_pcm_batch(blobs, sr=sr, stats=st0, feeders=1)
        for name, (y, r), (y0, r0) in zip(FILES, got, ref):
            want = pcm_by_rate[sr][name]
            assert r == r0 and y.shape == want.shape and np.array_equal(_bits(y), _bits(want)) and np.array_equal(_bits(y), _bits(y0)), (name, sr)
        assert idx == [None] * n and st0[5:] == st1[5:]
        for kw in (dict(mono=True), dict(mono=True, peak_normalize=True, preemphasis=A)):
            a = pcm.get_pcm_batch(blobs, sr=sr, **kw)
            b = pcm.get_pcm_batch(blobs, sr=sr, split_db=None, **kw)
            frames, chans, rts = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
            ib = _corpus.IntervalBuffers(lib, n)
            cond = pcm.cond_spec(kw.get("peak_normalize", False), kw.get("preemphasis"))
            c = _corpus.run(lib, lib.ogg_vorbis_pcm_corpus_split, blobs, (4, 2, 64, 0, sr or 0, 2, C.byref(cond), None), (frames, chans, rts, ib.ptrs, ib.counts),
                            lambda i, p: _corpus.copy_into(np.zeros(int(frames[i]), np.float32), p), pcm.PcmError, "raise", "pcm")
            assert not any(ib.ptrs) and not ib.counts.any()
            for (p, _), (q, _), r in zip(a, b, c):
                assert np.array_equal(_bits(p), _bits(q)) and p.shape == r.shape and np.array_equal(_bits(p), _bits(r))
        for kw in (E2E[0], E2E[1]):
            st0, st1, idx = [], [], []
            a = spectral.get_spectral_batch(blobs, sr=sr, stats=st0, feeders=1, **kw)
            b = spectral.get_spectral_batch(blobs, sr=sr, split_db=None, split_index=idx, stats=st1, feeders=1, **kw)
            assert idx == [None] * n and st0[5:] == st1[5:]
            s = spectral.spectral_spec(**kw)
            counts, joined = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
            ib = _corpus.IntervalBuffers(lib, n)
            dim = spectral.spec_dim(s)
            c = _corpus.run(lib, lib.ogg_vorbis_spectral_corpus_split, blobs, (4, 2, 64, 0, C.byref(s), sr or 0, None, None, None),
                            (counts, joined, ib.ptrs, ib.counts), lambda i, p: _corpus.copy_into(np.zeros((int(counts[i]), dim), np.float32), p),
                            spectral.SpectralError, "raise", "spectral")
            assert not any(ib.ptrs) and not ib.counts.any()
            for p, q, r in zip(a, b, c):
                assert np.array_equal(_bits(p), _bits(q)) and p.shape == r.shape and np.array_equal(_bits(p), _bits(r))
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
                off = g.pcm_split_host(None, cond, S, fmt=fmt)
                assert np.array_equal(off["pcm"].view(np.uint8), out.view(np.uint8)) and np.array_equal(off["frames"], frames)
                assert np.array_equal(_bits(off["peaks"]), _bits(peaks)) and not off["counts"].any() and not off["refs"].any()
            want = g.pcm_cond_spectral_host(cond, s, None, [44100] * S)
            off = g.pcm_split_spectral_host(None, cond, s, None, [44100] * S)
            assert np.array_equal(_bits(off["rows"]), _bits(want["rows"])) and np.array_equal(off["seg_rows"], want["seg_rows"])
            assert np.array_equal(_bits(off["peaks"]), _bits(want["peaks"])) and not off["counts"].any()
    finally:
        g.close()


@pytest.mark.parametrize("sr", [None, 16000])
def test_split_pcm_and_intervals_end_to_end(mods, blobs, sr):
    """On every fixture: get_intervals_batch equals the model on get_pcm_batch(mono=True)'s signal (its margin above the band);
    get_pcm_batch(mono=True, split_db=d, ...) is the concatenation of that signal's slices, bit for bit, and split_index those
    intervals; int16 is the existing conversion; with peak_normalize and preemphasis the result lies within the conditioning stage's
    gates (tests/test_gpu_condition.py: the peak exactly, y / p exactly, one FMA rounding) against tests/condition_model.py on the
    joined signal."""
    pcm, _ = mods
    planes = pcm.get_pcm_batch(blobs, sr=sr, mono=True)
    smallest, most = {}, 0
    for d, L, H in E2E_TRIM:
        kw = dict(sr=sr, mono=True, split_db=d, split_frame_length=L, split_hop_length=H)
        idx, idx2, tidx = [], [], ["x"]
        ivs = pcm.get_intervals_batch(blobs, d, L, H, sr=sr)
        got = pcm.get_pcm_batch(blobs, split_index=idx, trim_index=tidx, **kw)
        got16 = pcm.get_pcm_batch(blobs, dtype="int16", **kw)
        cnd = pcm.get_pcm_batch(blobs, peak_normalize=True, preemphasis=A, split_index=idx2, **kw)
        assert tidx == [None] * len(blobs)
        one = pcm.get_intervals_from_raw_bytes(blobs[0], d, frame_length=L, hop_length=H, sr=sr)
        assert np.array_equal(one[0], ivs[0][0]) and one[1:] == ivs[0][1:]
        for i, (name, data) in enumerate(zip(FILES, blobs)):
            y = planes[i][0]
            m = sm.split(y, d, L, H)
            smallest[(d, L, H)] = min(smallest.get((d, L, H), np.inf), m["margin"])
            assert m["margin"] > sm.band(L), (name, d, L, H, m["margin"])
            w = (name, sr, d, L, H, len(m["intervals"]))
            most = max(most, len(m["intervals"]))
            assert ivs[i][0].dtype == np.int64 and np.array_equal(ivs[i][0], m["intervals"]), w
            assert ivs[i][1] == (sr or _rate(data)) and ivs[i][2] == y.shape[0], w
            assert np.array_equal(idx[i], m["intervals"]) and np.array_equal(idx2[i], m["intervals"]), w
            assert got[i][1] == (sr or _rate(data)) and got[i][0].dtype == np.float32
            assert got[i][0].shape == m["joined"].shape and np.array_equal(_bits(got[i][0]), _bits(m["joined"])), w
            assert np.array_equal(got16[i][0], _s16(m["joined"])), w
            j, z = m["joined"], cnd[i][0]
            assert z.shape == j.shape, w
            p = np.abs(j).max() if j.shape[0] else np.float32(0.0)
            assert p == np.float32(cm.peak(j))
            y1 = j / p if p > 0 else j
            z64 = cm.preemphasis(y1.astype(np.float64), A)
            assert (np.abs(z.astype(np.float64) - z64) <= U * np.abs(z64)).all(), w
            if j.shape[0]:
                assert _bits(z[0]) == _bits(y1[0]), w
    assert most > 1
    print("split end to end (sr %s): most intervals %d, smallest margin per parameter set" % (sr, most),
          {k: float("%.3g" % v) for k, v in smallest.items()})


def test_split_spectral_rows_equal_the_model(mods, blobs):
    """get_spectral_batch(split_db=...) against tests/spectral_model.py on the device's own joined plane under GATE, unchanged; with
    delta=2, normalize="mean_var" under the post tests' composed gate, where a file joined below delta_width frames fails alone; with
    peak_normalize and preemphasis on top of the split as well."""
    pcm, spectral = mods
    worst = {}
    for sr, (d, L, H), kws in ((None, E2E_TRIM[0], E2E), (16000, E2E_TRIM[1], E2E[:1]), (None, E2E_TRIM[2], E2E[:1])):
        tk = dict(split_db=d, split_frame_length=L, split_hop_length=H)
        for cond in (dict(), dict(peak_normalize=True, preemphasis=A)):
            idx, idx2 = [], []
            planes = pcm.get_pcm_batch(blobs, sr=sr, mono=True, split_index=idx, **tk, **cond)
            for kw in kws:
                res = spectral.get_spectral_batch(blobs, sr=sr, split_index=idx2, **tk, **cond, **kw)
                assert all(np.array_equal(p, q) for p, q in zip(idx, idx2))
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
                assert short > 0  # the case is there: files joined below the delta width, failing alone
            worst["post/%s/%d" % (sr, L)] = max(worst.get("post/%s/%d" % (sr, L), 0.0), w)
    print("split rows, worst |d| / gate:", {k: round(v, 4) for k, v in sorted(worst.items())})


def test_host_entries_leave_the_pcm_and_the_next_submit_alone(mods, synth):
    """Every new host entry between two submits, and split, trim, split on one handle: vsyn_pcm_fetch_host and the next submit are
    bit-identical to a handle that made no such call; the split entries agree with each other, with vsyn_pcm_split_device on the
    fetched PCM, and give the same results before and after the trim call."""
    import torch
    from parseoggvorbis_amd.binding import Synth, VSYN_PCM_F32, VSYN_PCM_S16
    from tests.workloads import fixture_like_spec, synth_batch
    _, spectral = mods
    spec = fixture_like_spec(2)
    b1 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=21)
    b2 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=22)
    S, Cn = len(b1["segments"]), 2
    cond = _cond(True, A)
    split = _trim(3.0, 64, 16)
    s = spectral.spectral_spec(kind="mel_db", n_fft=64, hop_length=32, n_mels=8)
    outs = []
    for with_split in (False, True):
        g = Synth(spec, device=0, max_streams=4)
        try:
            assert g.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"], flags=4)["rc"] == 0
            f1, fr = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
            if with_split:
                only = g.pcm_split_intervals_host(split, S)
                plain = g.pcm_split_host(split, None, S)
                tr = g.pcm_trim_host(split, None, S)
                again = g.pcm_split_host(split, None, S)
                h32 = g.pcm_split_host(split, cond, S)
                h16 = g.pcm_split_host(split, cond, S, fmt=VSYN_PCM_S16)
                rows = g.pcm_split_spectral_host(split, cond, s, None, [16000] * S)
                only2 = g.pcm_split_intervals_host(split, S)
            f1b, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
            assert np.array_equal(f1, f1b)
            r2 = g.submit_host(b2["packets"], b2["segments"], b2["ys"], b2["residue"], b2["plane_stride"])
            assert r2["rc"] == 0
            outs.append((f1, r2["pcm"], r2["emit_len"]))
        finally:
            g.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    t_max = int(fr.max())
    x = np.zeros((S, Cn, t_max + 4), np.float32)
    for gi in range(S):
        x[gi, :, :int(fr[gi])] = f1[gi, :int(fr[gi])].T
    dev = _run_split(synth, split, x, [int(t) for t in fr])
    assert max(int(c) for c in dev["counts"]) > 1  # 3 dB under the loudest frame: pauses inside
    assert np.array_equal(only["frames"], fr.astype(np.uint64))
    for r in (only, plain, again, h32, h16, rows, only2):
        assert np.array_equal(r["counts"], dev["counts"]) and all(np.array_equal(p, q) for p, q in zip(r["intervals"], dev["iv"]))
        assert np.array_equal(r["refs"], dev["ref"])
    for gi in range(S):
        n = int(dev["n"][gi])
        assert (int(tr["bounds"][gi][0]), int(tr["bounds"][gi][1])) == (int(dev["iv"][gi][0, 0]), int(dev["iv"][gi][-1, 1]))
        for r in (plain, again):
            assert int(r["frames"][gi]) == n and np.array_equal(_bits(r["pcm"][gi, :n]), _bits(dev["out"][gi, :n])) and not r["pcm"][gi, n:].any()
        assert int(h32["frames"][gi]) == n == int(h16["frames"][gi]) == int(rows["frames"][gi])
        assert np.array_equal(h16["pcm"][gi, :n], _s16(h32["pcm"][gi, :n])) and not h32["pcm"][gi, n:].any() and not h16["pcm"][gi, n:].any()
        assert int(rows["seg_rows"][gi]) == int(synth.lib.vsyn_spectral_num_frames(C.byref(s), n))
    assert np.array_equal(_bits(rows["peaks"]), _bits(h32["peaks"])) and rows["rows"].shape[0] == int(rows["seg_rows"].sum())
    # the rows: the spectral stage alone on the conditioned joined plane
    d_cd = torch.from_numpy(np.ascontiguousarray(h32["pcm"])).cuda()
    d_n = torch.from_numpy(dev["n"].view(np.int32).copy()).cuda()
    d_rows = torch.full((rows["rows"].shape[0] + 2, 8), float("nan"), dtype=torch.float32, device="cuda")
    synth.spectral_device(s, [16000] * S, d_cd.data_ptr(), h32["pcm"].shape[1], 1, d_n.data_ptr(), d_rows.data_ptr(), None,
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(rows["rows"]), _bits(d_rows.cpu().numpy()[:rows["rows"].shape[0]]))
