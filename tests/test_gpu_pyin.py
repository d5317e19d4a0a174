"""pYIN on the GPU (vsyn_pyin_device, vsyn_pyin_decode_device, vsyn_pcm_pyin_host, ogg_vorbis_pyin_corpus, get_pyin_batch) against the
float64 model of tests/pyin_model.py.

Gates (derived in the model, not tuned on the device):
    frames       the model's count.
    states       vsyn_pyin_decode_device on the model's observations: equal to the model's on EVERY frame, and the path, scored with
                 the model's float64 tables, within twice the model's propagated bound E of its optimum. tests/test_pyin_cpu.py
                 asserts that every decision of every case is decided.
    voiced, bin  vsyn_pyin_device: the voiced flag and rint(12 bps log2(f0 / fmin)) equal on every frame; f0 equal to float32 of the
                 model's table value.
    voiced_prob  |d| <= (2^-24 + pbound + 4096 * 2^-53) * vp: one float32 rounding plus the model's relative bound on a P_k
                 (pyin_model.p_bound) and on the chain that adds at most 2049 of them.
"""
import ctypes as C
import time

import numpy as np
import pytest

from tests import pitch_cases as pc
from tests import pitch_model as pm
from tests import pyin_cases as yc
from tests import pyin_model as ym
from tests import trim_model as tm
from tests.test_gpu_condition import _bits, blobs, mods, pcm_by_rate, synth  # noqa: F401
from tests.test_gpu_spectral import FILES, _rate
from tests.test_gpu_trim import VARIANTS, _batch

pytestmark = pytest.mark.gpu

F32 = 2.0 ** -24


def _spec(g, **kw):
    from parseoggvorbis_amd import pitch
    a = dict(fmin=g["fmin"], fmax=g["fmax"], frame_length=g["L"], hop_length=g["H"], resolution=g["resolution"], n_thresholds=yc.N_THRESHOLDS)
    a.update(kw)
    return pitch.pyin_spec(**a)


def _run(g, spec, x, frames, rates, in_off=0, extra_rows=3):
    """vsyn_pyin_device over x (S, C, plane) float32 with frames [S] and rates [S]: dict(rows: a list of (F, 3) float32 arrays,
    off [S+1], refused [S]). Asserts that nothing behind the last row was written."""
    import torch
    S, Cn, plane = x.shape
    buf = torch.zeros(x.size + 8, dtype=torch.float32, device="cuda")
    buf[in_off:in_off + x.size].copy_(torch.from_numpy(np.ascontiguousarray(x).ravel()))
    d_frames = torch.from_numpy(np.asarray(frames, np.int64).astype(np.uint32).view(np.int32)).cuda()
    cap = sum(int(g.lib.vsyn_pyin_num_frames(C.byref(spec), min(int(t), plane))) for t in frames) + extra_rows
    d_rows = torch.full((cap, 3), -7.0, dtype=torch.float32, device="cuda")
    d_off = torch.full((S + 1,), -1, dtype=torch.int64, device="cuda")
    d_ref = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    g.pyin_device(spec, rates, buf.data_ptr() + 4 * in_off, plane, Cn, d_frames.data_ptr(), d_rows.data_ptr(), d_off.data_ptr(),
                  d_ref.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rows, off = d_rows.cpu().numpy(), d_off.cpu().numpy()
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] <= cap - extra_rows
    assert (rows[off[-1]:] == -7.0).all()
    return dict(rows=[rows[off[i]:off[i + 1]] for i in range(S)], off=off, refused=d_ref.cpu().numpy())


def _decode(g, spec, rates, obs_list):
    """vsyn_pyin_decode_device over the segments' dense (F, B) float64 rows: a list of (F,) state arrays. Asserts that nothing behind
    the last state was written."""
    import torch
    seg_rows = [o.shape[0] for o in obs_list]
    total = sum(seg_rows)
    flat = np.concatenate([o.reshape(-1) for o in obs_list] + [np.zeros(1)])
    d_obs = torch.from_numpy(flat).cuda()
    d_states = torch.full((total + 3,), -7, dtype=torch.int32, device="cuda")
    g.pyin_decode_device(spec, rates, d_obs.data_ptr(), seg_rows, d_states.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    st = d_states.cpu().numpy()
    assert (st[total:] == -7).all()
    off = np.concatenate([[0], np.cumsum(seg_rows)])
    return [st[off[i]:off[i + 1]].astype(np.int64) for i in range(len(obs_list))]


def _check_path(states, dec, what):
    assert np.array_equal(states, dec["states"]), (what, np.flatnonzero(states != dec["states"])[:5], states[:8], dec["states"][:8])
    if len(states):
        score = ym.path_score(states, dec["log_obs"], dec["lt"])
        assert score >= dec["score"] - 2 * dec["E"][-1], (what, score, dec["score"])


@pytest.mark.parametrize("group", list(yc.GROUPS))
def test_decode_alone_on_the_models_observations(synth, group):
    """vsyn_pyin_decode_device on the model's obs of every case of the group, all segments in one launch (two rates: two widths)."""
    idx = [i for i, c in enumerate(yc.cases()) if c["group"] == group]
    cases, models = [yc.cases()[i] for i in idx], [yc.models()[i] for i in idx]
    spec = _spec(yc.GROUPS[group])
    got = _decode(synth, spec, [c["sr"] for c in cases], [m["obs"] for m in models])
    for c, m, st in zip(cases, models, got):
        assert st.shape[0] == len(m["states"])
        if len(st):
            _check_path(st, m["dec"], (group, c["kind"], c["T"], c["sr"]))


def _crafted(B, h):
    """All zero; one bin at 1.0 that jumps by more than h; equal values across a symmetric pair of bins."""
    zero = np.zeros((6, B))
    jump = np.zeros((9, B))
    lo, hi = 1, min(B - 2, 1 + 2 * h + 3)
    jump[:4, lo] = 1.0
    jump[4:, hi] = 1.0
    pair = np.zeros((7, B))
    a, b = B // 2 - 1 - h // 2, B // 2 + 1 + h // 2
    pair[:, a] = pair[:, b] = 0.25  # (the two paths tie in every bit: the lower state wins, as in np.argmax)
    return dict(zero=zero, jump=jump, pair=pair), (lo, hi)


@pytest.mark.parametrize("group,sr", [("small", 8000), ("default", 22050), ("narrow", 8000)])
def test_decode_alone_on_crafted_rows(synth, group, sr):
    g = yc.GROUPS[group]
    spec = _spec(g)
    bps, B = ym.num_bins(g["fmin"], g["fmax"], g["resolution"])
    w = ym.width(sr, g["H"], 35.92, bps)
    rows, (lo, hi) = _crafted(B, w // 2)
    decs = {k: ym.decode(v, w, 0.01) for k, v in rows.items()}
    assert all(d["decided"] for d in decs.values()), [(k, [x for x in d["margins"] if not x[1] > x[2]][:2]) for k, d in decs.items()]
    if B > w:
        assert list(decs["jump"]["states"]) == [lo] * 4 + [hi] * 5 and hi - lo > w // 2  # the path leaves the band, voiced throughout
    got = _decode(synth, spec, [sr] * len(rows), list(rows.values()))
    for (k, d), st in zip(decs.items(), got):
        _check_path(st, d, (group, k))
    skipped = _decode(synth, spec, [sr, 0, sr], [rows["jump"], rows["zero"], rows["pair"]])  # a rate of 0 writes no state
    assert np.array_equal(skipped[0], decs["jump"]["states"]) and (skipped[1] == -7).all() and np.array_equal(skipped[2], decs["pair"]["states"])


def _check_rows(rows, m, c, what):
    """One segment's device rows against its model, frame by frame; returns the worst |d vp| / bound."""
    F = len(m["states"])
    assert rows.shape == (F, 3), (what, rows.shape, F)
    if F == 0:
        return 0.0
    f0, voiced, vp = rows[:, 0], rows[:, 1], rows[:, 2].astype(np.float64)
    assert np.isin(voiced, (0.0, 1.0)).all() and np.array_equal(voiced == 1.0, m["voiced"]), (what, np.flatnonzero((voiced == 1.0) != m["voiced"])[:5])
    bins = np.rint(12 * m["bps"] * np.log2(f0.astype(np.float64) / c["fmin"])).astype(np.int64)
    assert np.array_equal(bins, m["bins"]), (what, np.flatnonzero(bins != m["bins"])[:5], bins[:8], m["bins"][:8])
    assert np.array_equal(_bits(f0), _bits(m["f0"].astype(np.float32))), what
    bound = (F32 + m["pbound"] + 4096 * pm.U) * m["vp"]
    dv = np.abs(vp - m["vp"])
    assert (dv <= bound).all(), (what, float(dv.max()), np.flatnonzero(dv > bound)[:5])
    return float((dv / np.where(bound > 0, bound, 1.0)).max())


@pytest.mark.parametrize("group", list(yc.GROUPS))
def test_stage_alone_against_the_model(synth, group):
    """Every case of the group, grouped by channel count into one launch each (mixed rates and lengths in a batch), the stride /
    offset variants of the trim stage's test in rotation."""
    idx = [i for i, c in enumerate(yc.cases()) if c["group"] == group]
    cases, models = yc.cases(), yc.models()
    spec = _spec(yc.GROUPS[group])
    worst = 0.0
    for k, Cn in enumerate(pc.CHANNELS):
        sub = [i for i in idx if cases[i]["C"] == Cn]
        if not sub:
            continue
        odd, in_off, _ = VARIANTS[(k + list(yc.GROUPS).index(group)) % len(VARIANTS)]
        x, _ = _batch([np.zeros((Cn, 1), np.float32) if cases[i]["T"] == 0 else cases[i]["x"] for i in sub], odd)
        frames, rates = [cases[i]["T"] for i in sub], [cases[i]["sr"] for i in sub]
        got = _run(synth, spec, x, frames, rates, in_off)
        assert not got["refused"].any()
        for j, i in enumerate(sub):
            worst = max(worst, _check_rows(got["rows"][j], models[i], cases[i], (group, Cn, cases[i]["kind"], frames[j], rates[j])))
    print("pyin alone (%s): worst |d vp| / bound %.4f" % (group, worst))


def _same(a, b):
    return all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a["rows"], b["rows"])) and np.array_equal(a["off"], b["off"])


def test_exact_properties(synth):
    """No tolerance: a segment gives the same bits alone, in another slot of a batch, at an odd plane stride, at four alignments
    and in two runs; a rate of 0 and T = 0 give 0 rows; without centre padding the frame count is the spectral stage's."""
    for group in ("narrow", "small", "default"):
        g = yc.GROUPS[group]
        L, H = g["L"], g["H"]
        cases = [c for c in yc.cases() if c["group"] == group and c["C"] == 2 and c["T"] >= H]
        assert len(cases) >= 2
        x, frames = _batch([c["x"] for c in cases], False)
        rates = [c["sr"] for c in cases]
        spec = _spec(g)
        base = _run(synth, spec, x, frames, rates)
        assert _same(base, _run(synth, spec, x, frames, rates))
        order = list(range(len(frames)))[::-1]
        mixed = _run(synth, spec, x[order], [frames[j] for j in order], [rates[j] for j in order])
        for j, src in enumerate(order):
            assert np.array_equal(_bits(mixed["rows"][j]), _bits(base["rows"][src])), (group, src)
        alone = _run(synth, spec, x[1:2], frames[1:2], rates[1:2])
        assert np.array_equal(_bits(alone["rows"][0]), _bits(base["rows"][1]))
        odd = np.zeros((x.shape[0], 2, x.shape[2] + 3), np.float32)
        odd[:, :, :x.shape[2]] = x
        assert _same(_run(synth, spec, odd, frames, rates), base), (group, "odd stride")
        for off in (1, 2, 3):
            assert _same(_run(synth, spec, x, frames, rates, off), base), (group, off)
        skip = _run(synth, spec, x, [0] + frames[1:], rates[:-1] + [0])
        assert skip["rows"][0].shape[0] == 0 and skip["rows"][-1].shape[0] == 0
        assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(skip["rows"][1:-1], base["rows"][1:-1]))
        nc = _run(synth, _spec(g, center=False), x, frames, rates)
        for j, T in enumerate(frames):
            assert nc["rows"][j].shape[0] == pm.num_frames(T, L, H, False) == (0 if T < L else 1 + (T - L) // H)


def test_a_segment_that_is_not_finite_is_refused_alone(synth):
    """An Inf or a NaN in the middle, in the last sample, and (H > L) where no frame covers it: that segment's rows are NaN and
    its refused word 1; its neighbours' rows are unchanged bit for bit."""
    for (L, H), Cn in (((512, 128), 2), ((64, 200), 1)):
        segs = [pc.segment("glide", Cn, T, 22050, 900 + i, L) for i, T in enumerate((4097, 6011, 4097))]
        x, frames = _batch(segs, False)
        rates = [22050, 8000, 22050]
        spec = _spec(dict(L=L, H=H, fmin=400.0, fmax=2000.0, resolution=0.1))
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


def test_bad_specs_are_refused_with_nothing_launched(synth, mods, blobs):
    """Each invalid-spec case of step 10: VSYN_ERR_INVALID from the device and the decode entry and nothing written; the host entry
    and the corpus entry refuse the call."""
    import torch
    from parseoggvorbis_amd import _corpus, pitch
    from parseoggvorbis_amd.binding import Status, Synth, VsynError
    from tests.test_pyin_cpu import BAD_SPECS, _c_spec
    from tests.workloads import fixture_like_spec, synth_batch
    t = torch.full((256,), 5.0, dtype=torch.float32, device="cuda")
    f = torch.full((8,), 64, dtype=torch.int32, device="cuda")
    o = torch.full((64,), 9, dtype=torch.int32, device="cuda")
    d = torch.full((4096,), 0.25, dtype=torch.float64, device="cuda")
    cases = [(_c_spec(**kw), 8000 if kw.get("res") == 0.34 else 22050) for kw in BAD_SPECS]
    for spec, rate in cases:
        with pytest.raises(VsynError) as ei:
            synth.pyin_device(spec, [rate], t.data_ptr(), 64, 2, f.data_ptr(), t.data_ptr() + 512, o.data_ptr(), o.data_ptr() + 32)
        assert ei.value.code == 1, str(ei.value)
        with pytest.raises(VsynError) as ei:
            synth.pyin_decode_device(spec, [rate], d.data_ptr(), [2], o.data_ptr())
        assert ei.value.code == 1, str(ei.value)
    with pytest.raises(VsynError):
        synth.pyin_device(_c_spec(), [22050], t.data_ptr(), 64, 0, f.data_ptr(), t.data_ptr() + 512, o.data_ptr(), o.data_ptr() + 32)
    with pytest.raises(VsynError):
        synth.pyin_decode_device(_c_spec(), [22050], None, [2], o.data_ptr())
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == 5.0).all() and (o.cpu().numpy() == 9).all()
    bt = synth_batch(fixture_like_spec(2), streams=3, packets_per_stream=12, pattern="mixed", seed=31)
    S = len(bt["segments"])
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    try:
        assert g.submit_host(bt["packets"], bt["segments"], bt["ys"], bt["residue"], bt["plane_stride"], flags=4)["rc"] == 0
        for spec, rate in cases:
            rates = np.full(S, rate, np.uint32)
            seg_rows, rows, ref = np.full(S, 77, np.uint64), np.full((64, 3), 77.0, np.float32), np.full(S, 77, np.uint32)
            err = C.c_char_p()
            rc = g.lib.vsyn_pcm_pyin_host(g.h, C.byref(spec), S, rates.ctypes.data, 0, rows.ctypes.data, 64, seg_rows.ctypes.data, ref.ctypes.data,
                                          C.byref(Status()), C.byref(err))
            assert rc == 1 and err.value
            assert (seg_rows == 77).all() and (rows == 77).all() and (ref == 77).all()
    finally:
        g.close()
    lib = pitch._load()
    n = len(blobs)
    cnt, frames, rts = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    with pytest.raises(pitch.PyinError, match="invalid pyin spec"):
        _corpus.run(lib, lib.ogg_vorbis_pyin_corpus, blobs, (4, 2, 64, 0, 0, C.byref(_c_spec(L=3))), (cnt, frames, rts), lambda i, p: None,
                    pitch.PyinError, "raise", "pyin")


E2E = dict(fmin=150.0, fmax=600.0, frame_length=512, hop_length=256)


@pytest.mark.parametrize("sr", [None, 16000])
def test_get_pyin_batch_equals_the_model_on_the_fixtures(mods, blobs, sr):
    """get_pyin_batch on every Ogg fixture against the model applied to get_pcm_batch(mono=True, sr=sr) of the same files; fill_na
    as NaN, a number and None; a damaged file returns a PyinError in its slot only; get_pyin_from_raw_bytes is the one-file form."""
    from parseoggvorbis_amd import pitch
    pcm, _ = mods
    planes = pcm.get_pcm_batch(blobs, sr=sr, mono=True)
    broken = blobs[0][:len(blobs[0]) // 8]
    got = pitch.get_pyin_batch(list(blobs) + [broken], sr=sr, errors="return", fill_na=None, **E2E)
    assert isinstance(got[-1], pitch.PyinError) and not any(isinstance(r, Exception) for r in got[:-1])
    with pytest.raises(pitch.PyinError, match="file %d" % len(blobs)):
        pitch.get_pyin_batch(list(blobs) + [broken], sr=sr, **E2E)
    nan = pitch.get_pyin_batch(blobs, sr=sr, **E2E)
    num = pitch.get_pyin_batch(blobs, sr=sr, fill_na=-1.0, **E2E)
    one = pitch.get_pyin_from_raw_bytes(blobs[1], sr=sr, fill_na=None, **E2E)
    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip((one[0], one[2]), (got[1][0], got[1][2]))) and np.array_equal(one[1], got[1][1])
    worst = 0.0
    for name, data, (y, r), (f0, voiced, vp, rate), a, b in zip(FILES, blobs, planes, got, nan, num):
        assert rate == r == (sr or _rate(data)) and f0.dtype == vp.dtype == np.float32 and voiced.dtype == np.bool_ and f0.ndim == 1
        m = ym.pyin(y, rate, E2E["fmin"], E2E["fmax"], yc.beta(), E2E["frame_length"], E2E["hop_length"])
        assert m["decided"], (name, sr, [x for x in m["margins"] if not x[2] > x[3]][:3])
        rows = np.stack([f0, voiced.astype(np.float32), vp], axis=1)
        worst = max(worst, _check_rows(rows, m, E2E, (name, sr)))
        assert np.array_equal(a[1], voiced) and np.array_equal(b[1], voiced) and np.array_equal(_bits(a[2]), _bits(vp))
        assert np.isnan(a[0][~voiced]).all() and np.array_equal(_bits(a[0][voiced]), _bits(f0[voiced]))
        assert (b[0][~voiced] == -1.0).all() and np.array_equal(_bits(b[0][voiced]), _bits(f0[voiced]))
    print("pyin end to end (sr %s): worst |d vp| / bound %.4f" % (sr, worst))


def test_host_entry_equals_the_device_entry_and_leaves_the_pcm_alone(synth):
    """vsyn_pcm_pyin_host between two submits: vsyn_pcm_fetch_host and the next submit are bit-identical to a handle that made no
    such call; its rows are vsyn_pyin_device's on the fetched PCM; behind the resampler the rows are finite."""
    from parseoggvorbis_amd import pitch
    from parseoggvorbis_amd.binding import Synth, VSYN_PCM_F32
    from tests.workloads import fixture_like_spec, synth_batch
    spec = fixture_like_spec(2)
    b1 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=21)
    b2 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=22)
    S = len(b1["segments"])
    ps = pitch.pyin_spec(600.0, 2000.0, 64, 16)
    rates = [16000, 0, 8000][:S] + [16000] * max(0, S - 3)
    outs = []
    for with_pyin in (False, True):
        g = Synth(spec, device=0, max_streams=4)
        try:
            assert g.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"], flags=4)["rc"] == 0
            f1, fr = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
            if with_pyin:
                host = g.pcm_pyin_host(ps, rates)
                again = g.pcm_pyin_host(ps, rates)
                low = g.pcm_pyin_host(ps, rates, 12000)
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


def test_timing_of_the_default_shape(synth):
    """The timing case, not a per-value case: 64 mono segments of 10 s at 22050 Hz, the defaults, timed after a warm-up launch, next
    to YIN on the same input in the same run. Printed; nothing is asserted on the times."""
    import torch
    from parseoggvorbis_amd import pitch
    S, T, sr = 64, 220500, 22050
    y = yc.tone(T, sr, (220.0, 440.0, 330.0, 262.0), 9999)
    x = np.ascontiguousarray(np.broadcast_to(y, (S, 1, T)))
    buf = torch.from_numpy(x).cuda()
    d_frames = torch.full((S,), T, dtype=torch.int32, device="cuda")
    py = pitch.pyin_spec(yc.C2, yc.C7)
    yi = pitch.pitch_spec(yc.C2, yc.C7)
    F = int(synth.lib.vsyn_pyin_num_frames(C.byref(py), T))
    rows3 = torch.zeros((S * F, 3), dtype=torch.float32, device="cuda")
    rows2 = torch.zeros((S * F, 2), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    times = {}
    for name, call in (("pyin", lambda: synth.pyin_device(py, [sr] * S, buf.data_ptr(), T, 1, d_frames.data_ptr(), rows3.data_ptr(), None, None, stream)),
                       ("yin", lambda: synth.pitch_device(yi, [sr] * S, buf.data_ptr(), T, 1, d_frames.data_ptr(), rows2.data_ptr(), None, None, stream))):
        call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times[name] = time.perf_counter() - t0
    r = rows3.cpu().numpy().reshape(S, F, 3)
    assert F == 431 and np.isfinite(r).all() and np.array_equal(_bits(r[0]), _bits(r[S - 1])) and (r[0, :, 1] == 1.0).any()
    print("pyin timing (64 x 10 s mono at 22050 Hz, defaults, F = %d): pyin %.2f ms, yin %.2f ms (one measurement each, wall time of the second launch)"
          % (F, 1e3 * times["pyin"], 1e3 * times["yin"]))
