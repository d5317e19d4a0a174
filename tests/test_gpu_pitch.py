"""Pitch on the GPU (vsyn_pitch_device, vsyn_pcm_pitch_host, ogg_vorbis_pitch_corpus, get_f0_batch) against the float64 model of
tests/pitch_model.py.

Gates per frame (derived in the model, not tuned on the device):
    frames     the model's count.
    lag        round(sr / f0 - the model's shift) equals the model's p_min + i*, on EVERY frame: tests/test_pitch_cpu.py asserts that
               every frame of every case decides by a margin above pitch_model.band.
    c[i*]      |d| <= (2^-24 + band) * c: one float32 rounding plus the band.
    f0         |d| <= (tol + 2^-24) * f0, tol = pitch_model.f0_tolerance of the frame (from band, |a| and the period).
"""
import ctypes as C

import numpy as np
import pytest

from tests import pitch_cases as pc
from tests import pitch_model as pm
from tests import trim_model as tm
from tests.test_gpu_condition import _bits, blobs, mods, pcm_by_rate, synth  # noqa: F401
from tests.test_gpu_spectral import FILES, _rate
from tests.test_gpu_trim import VARIANTS, _batch

pytestmark = pytest.mark.gpu

F32 = 2.0 ** -24


def _spec(fmin, fmax, L=2048, H=512, thr=pc.THRESHOLD, center=True):
    from parseoggvorbis_amd.binding import PitchSpec
    return PitchSpec(L, H, 1 if center else 0, 0, fmin, fmax, thr)


def _run(g, spec, x, frames, rates, in_off=0, extra_rows=3):
    """vsyn_pitch_device over x (S, C, plane) float32 with frames [S] and rates [S]: dict(rows: a list of (F, 2) float32 arrays,
    off [S+1], refused [S]). Asserts that nothing behind the last row was written."""
    import torch
    S, Cn, plane = x.shape
    buf = torch.zeros(x.size + 8, dtype=torch.float32, device="cuda")
    buf[in_off:in_off + x.size].copy_(torch.from_numpy(np.ascontiguousarray(x).ravel()))
    d_frames = torch.from_numpy(np.asarray(frames, np.int64).astype(np.uint32).view(np.int32)).cuda()
    cap = sum(int(g.lib.vsyn_pitch_num_frames(C.byref(spec), min(int(t), plane))) for t in frames) + extra_rows
    d_rows = torch.full((cap, 2), -7.0, dtype=torch.float32, device="cuda")
    d_off = torch.full((S + 1,), -1, dtype=torch.int64, device="cuda")
    d_ref = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    g.pitch_device(spec, rates, buf.data_ptr() + 4 * in_off, plane, Cn, d_frames.data_ptr(), d_rows.data_ptr(), d_off.data_ptr(),
                   d_ref.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rows, off = d_rows.cpu().numpy(), d_off.cpu().numpy()
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] <= cap - extra_rows
    assert (rows[off[-1]:] == -7.0).all()
    return dict(rows=[rows[off[i]:off[i + 1]] for i in range(S)], off=off, refused=d_ref.cpu().numpy())


def _check_rows(rows, m, sr, what):
    """One segment's device rows against its model, frame by frame; returns the worst |d f0| / bound."""
    F = len(m["f0"])
    assert rows.shape == (F, 2), (what, rows.shape, F)
    if F == 0:
        return 0.0
    f0, c = rows[:, 0].astype(np.float64), rows[:, 1].astype(np.float64)
    lag = np.rint(sr / f0 - m["shift"]).astype(np.int64)
    assert np.array_equal(lag, m["lag"]), (what, np.flatnonzero(lag != m["lag"])[:5], lag[lag != m["lag"]][:5], m["lag"][lag != m["lag"]][:5])
    dc = np.abs(c - m["c"])
    assert (dc <= (F32 + m["band"]) * m["c"]).all(), (what, float(dc.max()))
    bound = (m["tol"] + F32) * m["f0"]
    df = np.abs(f0 - m["f0"])
    assert (df <= bound).all(), (what, float((df / bound).max()))
    return float((df / bound).max())


@pytest.mark.parametrize("L,H", pc.LH)
def test_stage_alone_against_the_model(synth, L, H):
    """Every case of tests/pitch_cases.py for (L, H), grouped by channel count into one launch each (mixed rates and lengths in a
    batch), the stride / offset variants of the trim stage's test in rotation."""
    cases, models = pc.cases(L, H), pc.models(L, H)
    worst = 0.0
    for k, Cn in enumerate(pc.CHANNELS):
        idx = [i for i, c in enumerate(cases) if c["C"] == Cn]
        odd, in_off, _ = VARIANTS[(k + pc.LH.index((L, H))) % len(VARIANTS)]
        x, frames = _batch([np.zeros((Cn, 1), np.float32) if cases[i]["T"] == 0 else cases[i]["x"] for i in idx], odd)
        frames = [cases[i]["T"] for i in idx]
        rates = [cases[i]["sr"] for i in idx]
        assert len(set(rates)) > 1
        if L < 64:  # fmin = sr / 8 and fmax = sr / 2 differ per rate: one launch per rate
            for r in sorted(set(rates)):
                sub = [j for j, i in enumerate(idx) if cases[i]["sr"] == r]
                got = _run(synth, _spec(r / 8.0, r / 2.0, L, H), x[sub], [frames[j] for j in sub], [r] * len(sub), in_off)
                assert not got["refused"].any()
                for j, rows in zip(sub, got["rows"]):
                    worst = max(worst, _check_rows(rows, models[idx[j]], r, (L, H, Cn, cases[idx[j]]["kind"], frames[j])))
            continue
        spec = _spec(cases[idx[0]]["fmin"], cases[idx[0]]["fmax"], L, H)  # (L >= 64: one band for the three rates)
        assert all(pm.periods(cases[i]["sr"], spec.fmin, spec.fmax, L) == (models[i]["p_min"], models[i]["p_max"]) for i in idx)
        got = _run(synth, spec, x, frames, rates, in_off)
        assert not got["refused"].any()
        for j, i in enumerate(idx):
            worst = max(worst, _check_rows(got["rows"][j], models[i], rates[j], (L, H, Cn, cases[i]["kind"], frames[j], rates[j])))
    print("pitch alone (L %d, H %d): worst |d f0| / bound %.4f" % (L, H, worst))


def _same(a, b):
    return all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a["rows"], b["rows"])) and np.array_equal(a["off"], b["off"])


def test_exact_properties(synth):
    """No tolerance: a segment gives the same bits alone, in another slot of a batch, at an odd plane stride, at four alignments
    and in two runs; a rate of 0 and T = 0 give 0 rows; without centre padding the frame count is the spectral stage's."""
    for (L, H) in ((512, 128), (64, 16), (2048, 512)):
        cases = [c for c in pc.cases(L, H) if c["C"] == 2 and c["T"] >= H]
        x, frames = _batch([c["x"] for c in cases], False)
        rates = [c["sr"] for c in cases]
        spec = _spec(cases[0]["fmin"], min(c["fmax"] for c in cases), L, H)
        base = _run(synth, spec, x, frames, rates)
        assert _same(base, _run(synth, spec, x, frames, rates))
        order = list(range(len(frames)))[::-1]
        mixed = _run(synth, spec, x[order], [frames[j] for j in order], [rates[j] for j in order])
        for j, src in enumerate(order):
            assert np.array_equal(_bits(mixed["rows"][j]), _bits(base["rows"][src])), (L, H, src)
        alone = _run(synth, spec, x[1:2], frames[1:2], rates[1:2])
        assert np.array_equal(_bits(alone["rows"][0]), _bits(base["rows"][1]))
        odd = np.zeros((x.shape[0], 2, x.shape[2] + 3), np.float32)
        odd[:, :, :x.shape[2]] = x
        assert _same(_run(synth, spec, odd, frames, rates), base), (L, H, "odd stride")
        for off in (1, 2, 3):
            assert _same(_run(synth, spec, x, frames, rates, off), base), (L, H, off)
        skip = _run(synth, spec, x, [0] + frames[1:], rates[:-1] + [0])
        assert skip["rows"][0].shape[0] == 0 and skip["rows"][-1].shape[0] == 0
        assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(skip["rows"][1:-1], base["rows"][1:-1]))
        nc = _run(synth, _spec(spec.fmin, spec.fmax, L, H, center=False), x, frames, rates)
        for j, T in enumerate(frames):
            assert nc["rows"][j].shape[0] == pm.num_frames(T, L, H, False) == (0 if T < L else 1 + (T - L) // H)
            y = tm.downmix(cases[j]["x"])
            m = pm.yin(y, rates[j], spec.fmin, spec.fmax, L, H, pc.THRESHOLD, False)
            if (m["margin"] > m["band"]).all():
                _check_rows(nc["rows"][j], m, rates[j], (L, H, "no centre", j))


def test_a_segment_that_is_not_finite_is_refused_alone(synth):
    """An Inf or a NaN in the middle, in the last sample, and (H > L) where no frame covers it: that segment's rows are NaN and
    its refused word 1; its neighbours' rows are unchanged bit for bit."""
    for (L, H), Cn in (((512, 128), 2), ((64, 200), 1)):
        segs = [pc.segment("glide", Cn, T, 22050, 900 + i, L) for i, T in enumerate((4097, 6011, 4097))]
        x, frames = _batch(segs, False)
        rates = [22050, 8000, 22050]
        spec = _spec(200.0, 4000.0, L, H)
        want = _run(synth, spec, x, frames, rates)
        assert not want["refused"].any() and all(np.isfinite(r).all() for r in want["rows"])
        spots = [("middle", 3000), ("last", 6010)] + ([("uncovered", 3 * H - L // 2 + L + 5)] if H > L else [])
        for value in (np.inf, -np.inf, np.nan):
            for name, t in spots:
                bad = x.copy()
                bad[1, Cn - 1, t] = value
                got = _run(synth, spec, bad, frames, rates)
                w = (L, H, value, name)
                assert list(got["refused"]) == [0, 1, 0], w
                assert got["rows"][1].shape == want["rows"][1].shape and np.isnan(got["rows"][1]).all(), w
                for gi in (0, 2):
                    assert np.array_equal(_bits(got["rows"][gi]), _bits(want["rows"][gi])), w


BAD_SPECS = [dict(L=3), dict(L=8193), dict(H=0), dict(fmin=0.0), dict(fmin=-5.0), dict(fmin=500.0, fmax=400.0), dict(fmin=float("nan")),
             dict(fmax=float("inf")), dict(fmax=11026.0), dict(thr=0.0), dict(thr=1.01), dict(thr=float("nan")), dict(options=2)]


def _bad(kw):
    from parseoggvorbis_amd.binding import PitchSpec
    a = dict(L=2048, H=512, options=1, fmin=65.0, fmax=2093.0, thr=0.1)
    a.update(kw)
    return PitchSpec(a["L"], a["H"], a["options"], 0, a["fmin"], a["fmax"], a["thr"])


def test_bad_specs_are_refused_with_nothing_launched(synth, mods, blobs):
    """Each invalid-spec case of step 10: VSYN_ERR_INVALID from both entry points and nothing written; the corpus entry refuses the
    call; Python refuses before the library is touched."""
    import torch
    from parseoggvorbis_amd import _corpus, pitch
    from parseoggvorbis_amd.binding import Status, Synth, VsynError
    from tests.workloads import fixture_like_spec, synth_batch
    t = torch.full((256,), 5.0, dtype=torch.float32, device="cuda")
    f = torch.full((8,), 64, dtype=torch.int32, device="cuda")
    o = torch.full((64,), 9, dtype=torch.int32, device="cuda")

    def device(spec, rate=22050, channels=2):
        try:
            synth.pitch_device(spec, [rate], t.data_ptr(), 64, channels, f.data_ptr(), t.data_ptr() + 512, o.data_ptr(), o.data_ptr() + 32)
        finally:
            torch.cuda.synchronize()
            assert (t.cpu().numpy() == 5.0).all() and (o.cpu().numpy() == 9).all()
    # (the last: 8000 Hz and L = 6 leave the one lag 2, n = 1)
    cases = [(_bad(kw), 22050) for kw in BAD_SPECS] + [(_bad(dict(fmin=3000.0, fmax=4000.0, L=6)), 8000)]
    for spec, rate in cases:
        with pytest.raises(VsynError) as ei:
            device(spec, rate)
        assert ei.value.code == 1, str(ei.value)
    with pytest.raises(VsynError):
        device(_bad({}), 22050, 0)
    assert synth.lib.vsyn_pitch_num_frames(C.byref(_bad(dict(L=3))), 1000) == 0
    assert synth.lib.vsyn_pitch_num_frames(C.byref(_bad({})), 1000) == 2 and synth.lib.vsyn_pitch_num_frames(C.byref(_bad({})), 0) == 0
    bt = synth_batch(fixture_like_spec(2), streams=3, packets_per_stream=12, pattern="mixed", seed=31)
    S = len(bt["segments"])
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    try:
        assert g.submit_host(bt["packets"], bt["segments"], bt["ys"], bt["residue"], bt["plane_stride"], flags=4)["rc"] == 0
        for spec, rate in cases:
            rates = np.full(S, rate, np.uint32)
            seg_rows, rows, ref = np.full(S, 77, np.uint64), np.full((64, 2), 77.0, np.float32), np.full(S, 77, np.uint32)
            err = C.c_char_p()
            rc = g.lib.vsyn_pcm_pitch_host(g.h, C.byref(spec), S, rates.ctypes.data, 0, rows.ctypes.data, 64, seg_rows.ctypes.data, ref.ctypes.data,
                                           C.byref(Status()), C.byref(err))
            assert rc == 1 and err.value
            assert (seg_rows == 77).all() and (rows == 77).all() and (ref == 77).all()
    finally:
        g.close()
    lib = pitch._load()
    n = len(blobs)
    cnt, frames, rts = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    with pytest.raises(pitch.PitchError, match="invalid pitch spec"):
        _corpus.run(lib, lib.ogg_vorbis_pitch_corpus, blobs, (4, 2, 64, 0, 0, C.byref(_bad(dict(L=3)))), (cnt, frames, rts), lambda i, p: None,
                    pitch.PitchError, "raise", "pitch")
    with pytest.raises(pitch.PitchError):
        pitch.get_f0_batch(blobs, 0.0, 2093.0)


E2E = dict(fmin=150.0, fmax=3000.0, frame_length=512, hop_length=160)


@pytest.mark.parametrize("sr", [None, 16000])
def test_get_f0_batch_equals_the_model_on_the_fixtures(mods, blobs, sr):
    """get_f0_batch on every Ogg fixture against the model applied to get_pcm_batch(mono=True, sr=sr) of the same files; a damaged
    file returns a PitchError in its slot only; get_f0_from_raw_bytes is the one-file form."""
    from parseoggvorbis_amd import pitch
    pcm, _ = mods
    planes = pcm.get_pcm_batch(blobs, sr=sr, mono=True)
    broken = blobs[0][:len(blobs[0]) // 8]
    got = pitch.get_f0_batch(list(blobs) + [broken], sr=sr, errors="return", **E2E)
    assert isinstance(got[-1], pitch.PitchError) and not any(isinstance(r, Exception) for r in got[:-1])
    with pytest.raises(pitch.PitchError, match="file %d" % len(blobs)):
        pitch.get_f0_batch(list(blobs) + [broken], sr=sr, **E2E)
    one = pitch.get_f0_from_raw_bytes(blobs[1], sr=sr, **E2E)
    assert np.array_equal(_bits(one[0]), _bits(got[1][0])) and np.array_equal(_bits(one[1]), _bits(got[1][1])) and one[2] == got[1][2]
    least, worst = np.inf, 0.0
    for name, data, (y, r), (f0, c, rate) in zip(FILES, blobs, planes, got):
        assert rate == r == (sr or _rate(data)) and f0.dtype == c.dtype == np.float32 and f0.ndim == 1
        m = pm.yin(y, rate, E2E["fmin"], E2E["fmax"], E2E["frame_length"], E2E["hop_length"], 0.1, True)
        if len(m["f0"]):
            least = min(least, float(m["margin"].min()))
            assert (m["margin"] > m["band"]).all(), (name, sr, float(m["margin"].min()))
        worst = max(worst, _check_rows(np.stack([f0, c], axis=1), m, rate, (name, sr)))
    print("pitch end to end (sr %s): smallest margin %.3g, worst |d f0| / bound %.4f" % (sr, least, worst))


def test_rate_that_does_not_fit_fails_alone(mods, blobs):
    """fmax above a file's sr / 2 is that file's error: rewritten to 8000 Hz, one fixture fails and the others are unchanged."""
    from parseoggvorbis_amd import pitch
    from tests.test_gpu_spectral import _rehead
    kw = dict(fmin=150.0, fmax=5000.0, frame_length=512, hop_length=160)
    want = pitch.get_f0_batch(blobs[:3], **kw)
    got = pitch.get_f0_batch([blobs[0], _rehead(blobs[1], 8000), blobs[2]], errors="return", **kw)
    assert isinstance(got[1], pitch.PitchError) and "sample rate 8000" in str(got[1])
    for i in (0, 2):
        assert np.array_equal(_bits(got[i][0]), _bits(want[i][0])) and np.array_equal(_bits(got[i][1]), _bits(want[i][1]))


def test_host_entry_leaves_the_pcm_and_the_next_submit_alone(mods, synth, blobs, pcm_by_rate):
    """vsyn_pcm_pitch_host between two submits: vsyn_pcm_fetch_host and the next submit are bit-identical to a handle that made no
    such call; its rows are vsyn_pitch_device's on the fetched PCM, natively and behind the resampler's plane; get_pcm_batch and
    get_spectral_batch with their defaults are unchanged by a pitch run in between."""
    from parseoggvorbis_amd import pitch
    from parseoggvorbis_amd.binding import Synth, VSYN_PCM_F32
    from tests.workloads import fixture_like_spec, synth_batch
    pcm, spectral = mods
    spec = fixture_like_spec(2)
    b1 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=21)
    b2 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=22)
    S = len(b1["segments"])
    ps = _spec(300.0, 4000.0, 64, 16)
    rates = [16000, 0, 8000][:S] + [16000] * max(0, S - 3)
    outs = []
    for with_pitch in (False, True):
        g = Synth(spec, device=0, max_streams=4)
        try:
            assert g.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"], flags=4)["rc"] == 0
            f1, fr = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
            if with_pitch:
                host = g.pcm_pitch_host(ps, rates)
                again = g.pcm_pitch_host(ps, rates)
                low = g.pcm_pitch_host(ps, rates, 12000)
            f1b, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
            assert np.array_equal(f1, f1b)
            r2 = g.submit_host(b2["packets"], b2["segments"], b2["ys"], b2["residue"], b2["plane_stride"])
            assert r2["rc"] == 0
            outs.append((f1, r2["pcm"], r2["emit_len"]))
        finally:
            g.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    t_max = int(fr.max())
    x = np.zeros((S, 2, t_max + 4), np.float32)
    for gi in range(S):
        x[gi, :, :int(fr[gi])] = f1[gi, :int(fr[gi])].T
    dev = _run(synth, ps, x, [int(t) for t in fr], rates)
    assert host["rc"] == 0 and not host["refused"].any() and int(host["seg_rows"][1]) == 0 and int(host["seg_rows"].sum()) > 0
    assert np.array_equal(host["seg_rows"], np.diff(dev["off"]).astype(np.uint64))
    assert np.array_equal(_bits(host["rows"]), _bits(np.concatenate(dev["rows"]))) and np.array_equal(_bits(again["rows"]), _bits(host["rows"]))
    assert int(low["seg_rows"][1]) == 0 and low["rows"].shape[0] == int(low["seg_rows"].sum()) > 0 and np.isfinite(low["rows"]).all()
    before = pcm.get_pcm_batch(blobs[:4]), spectral.get_spectral_batch(blobs[:4])
    pitch.get_f0_batch(blobs[:4], **E2E)
    after = pcm.get_pcm_batch(blobs[:4]), spectral.get_spectral_batch(blobs[:4])
    for name, (y0, r0), (y1, r1), s0, s1 in zip(FILES, before[0], after[0], before[1], after[1]):
        assert r0 == r1 and np.array_equal(_bits(y0), _bits(y1)) and np.array_equal(_bits(y0), _bits(pcm_by_rate[None][name]))
        assert np.array_equal(_bits(s0), _bits(s1))
