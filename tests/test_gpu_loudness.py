"""The loudness stage on the device (include/vorbis_synth_hip.h, "loudness") against the float64 model of tests/loudness_model.py.

Every gate is the bound of DESIGN.md 6m (tests/loudness_model.py bounds(), sample_bound(), block_bounds()), nothing fitted: per
K-weighted sample |d| <= (seq + dev) max|x|, the model's and the device's halves; per block mean and per gated mean what follows
from it through 2 |y| |dy| + dy^2 and (n + 1) 2^-53 per ordered sum. Every input asserts that each of its blocks is further from
both thresholds than its bound, so the device must keep exactly the model's blocks. The gain is numpy's
float32(sqrt(Z_t / zbar)) from the device's own zbar, and the scaled plane float32(x * g), both bit for bit.

(1) the stage alone, three rates x one and two channels x both channel modes, one call carrying every length at which the code
takes another path; (2) same PCM, same bits, wherever the segment lies; (3) refusals with the outputs untouched; (4) the host form
behind a submit; (5) get_loudness_batch end to end on the fixtures."""
import numpy as np
import pytest

from tests import loudness_model as lm

pytestmark = pytest.mark.gpu

KINDS = ("noise", "dc", "gated", "zeros")
TARGET = -23.0


@pytest.fixture(scope="module")
def synth():
    import torch
    assert torch.cuda.is_available()
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    yield g
    g.close()


def _spec(target=TARGET, mono=False, options=None):
    from parseoggvorbis_amd import binding
    opts = (binding.VSYN_LOUD_NORMALIZE if target is not None else 0) if options is None else options
    return binding.LoudnessSpec(opts, binding.VSYN_LOUD_MONO if mono else binding.VSYN_LOUD_SUM, 0.0 if target is None else target)


def _run_stage(g, spec, segs, rates, plane=None, outputs=True):
    """vsyn_loudness_device over segs (list of (C, T) float32): dict(rec, z [per segment], y [per segment] (Cs, T) float64, scaled
    [per segment] (Cs, T) float32). The planes are NaN behind every segment's frames and must stay so in the outputs."""
    import torch
    from parseoggvorbis_amd import binding
    S, C = len(segs), segs[0].shape[0]
    Cs = 1 if spec.channel_mode == binding.VSYN_LOUD_MONO else C
    frames = [s.shape[1] for s in segs]
    plane = plane or max(frames) + 5
    pcm = np.full((S, C, plane), np.nan, np.float32)
    for i, s in enumerate(segs):
        pcm[i, :, :frames[i]] = s
    nb = [lm.num_blocks(r, t) for r, t in zip(rates, frames)]
    d_pcm = torch.from_numpy(pcm).cuda()
    d_rec = torch.zeros(S * 40, dtype=torch.uint8, device="cuda")
    d_z = torch.full((sum(nb) + 3,), float("nan"), dtype=torch.float64, device="cuda")
    d_y = torch.full((S, Cs, plane), float("nan"), dtype=torch.float64, device="cuda") if outputs else None
    d_s = torch.full((S, Cs, plane), float("nan"), dtype=torch.float32, device="cuda") if outputs and spec.options else None
    try:
        g.loudness_device(spec, rates, frames, d_pcm.data_ptr(), plane, C, d_rec.data_ptr(), d_z.data_ptr(),
                          d_y.data_ptr() if outputs else None, plane, None if d_s is None else d_s.data_ptr(), plane,
                          torch.cuda.current_stream().cuda_stream)
    finally:
        torch.cuda.synchronize()
    rec = d_rec.cpu().numpy().view(binding.LOUDNESS_RECORD_DTYPE)
    z = d_z.cpu().numpy()
    assert np.isnan(z[sum(nb):]).all()
    out = dict(rec=rec, z=np.split(z[:sum(nb)], np.cumsum(nb)[:-1]) if S else [])
    for name, d in (("y", d_y), ("scaled", d_s)):
        if d is not None:
            a = d.cpu().numpy()
            for i, t in enumerate(frames):
                assert np.isnan(a[i, :, t:]).all(), (name, i)  # nothing written past a segment's frames
            out[name] = [a[i, :, :t] for i, t in enumerate(frames)]
    return out


def _check_segment(i, x, fs, mono, rec, z, y, scaled, worst):
    """One segment of a call against the model; worst collects the largest ratios to the bounds."""
    xs = lm.downmix(x) if mono else x
    m = lm.measure(x, fs, mono=mono)
    X = float(np.abs(xs[np.isfinite(xs)]).max()) if xs.size and np.isfinite(xs).any() else 0.0
    assert rec["status"] == m["status"], (i, rec, m["status"])
    assert rec["blocks"] == m["blocks"], i
    if m["status"] in (lm.NOT_FINITE, lm.RATE_REFUSED):
        assert rec["zbar"] == 0 and rec["zbar_a"] == 0 and rec["gain"] == 0 and rec["blocks_abs"] == 0 and rec["blocks_rel"] == 0
        if scaled is not None:
            assert not scaled.any()
        return
    if y is not None and xs.shape[1]:
        D = lm.sample_bound(fs, X)
        d = float(np.abs(y - m["y"]).max())
        assert d <= D, (i, d, D)
        if D:
            worst["y"] = max(worst["y"], d / D)
    assert lm.margins_exceed(m, fs, X), (i, "an input of this test lies within its bound of a threshold")
    Bz, Bza, Bzbar = lm.block_bounds(m, fs, X)
    assert len(z) == m["blocks"]
    if len(z):
        assert (np.abs(z - m["z"]) <= Bz).all(), i
        nz = Bz > 0
        if nz.any():
            worst["z"] = max(worst["z"], float((np.abs(z - m["z"])[nz] / Bz[nz]).max()))
    assert (rec["blocks_abs"], rec["blocks_rel"]) == (m["blocks_abs"], m["blocks_rel"]), i
    assert abs(rec["zbar_a"] - m["zbar_a"]) <= Bza and abs(rec["zbar"] - m["zbar"]) <= Bzbar, i
    if m["status"] == lm.OK:
        worst["zbar"] = max(worst["zbar"], abs(rec["zbar"] - m["zbar"]) / Bzbar)
        g = lm.gain(rec["zbar"], TARGET)
        assert rec["gain"].tobytes() == g.tobytes(), (i, rec["gain"], g)  # bit for bit from the device's own zbar
        if scaled is not None:
            assert np.array_equal(scaled, xs * g), i
    else:
        assert rec["zbar"] == 0 and rec["gain"] == 0
        if scaled is not None:
            assert not scaled.any()


def _batch(fs, C, seed):
    """The segments of one call: every length of lm.seg_lengths with the four signals in turn, a few seconds of each, and an Inf in
    a hop and a NaN in the tail behind the last whole hop between finite neighbours."""
    segs = [lm.signal(KINDS[i % 4], C, T, seed + i) for i, T in enumerate(lm.seg_lengths(fs))]
    T = int(2.3 * fs) + 7
    segs += [lm.signal(k, C, T, seed + 40 + i) for i, k in enumerate(("noise", "dc", "gated", "zeros"))]
    bad = lm.signal("noise", C, T, seed + 50)
    bad[C - 1, fs // 2 + 3] = np.inf
    segs.append(bad)
    segs.append(lm.signal("noise", C, T, seed + 51))
    bad = lm.signal("dc", C, T, seed + 52)
    assert T - 2 >= (lm.num_hops(fs, T) * fs) // 10
    bad[0, T - 2] = np.nan
    segs.append(bad)
    segs.append(lm.signal("dc", C, lm.TILE + 9, seed + 53))
    return segs


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("fs", lm.RATES)
def test_stage_alone_against_the_model(synth, fs, C):
    """(1) Measured on the MI355X: see DESIGN.md 6m for the worst ratio to each bound per rate and channel count."""
    segs = _batch(fs, C, 1000 * C + fs % 97)
    rates = [fs] * len(segs)
    rates[4] = 3999  # a refused rate among the others
    for mono in ((False,) if C == 1 else (False, True)):
        out = _run_stage(synth, _spec(mono=mono), segs, rates, plane=max(s.shape[1] for s in segs) + (4 if mono else 5))
        worst = dict(y=0.0, z=0.0, zbar=0.0)
        for i, x in enumerate(segs):
            _check_segment(i, x, rates[i], mono, out["rec"][i], out["z"][i], out["y"][i], out["scaled"][i], worst)
        print("stage alone, %d Hz, C %d, %s: worst ratio to the bound: samples %.3g, block means %.3g, zbar %.3g" %
              (fs, C, "mono" if mono else "sum", worst["y"], worst["z"], worst["zbar"]))
        assert worst["y"] > 0  # the comparison is not vacuous
        statuses = set(int(r["status"]) for r in out["rec"])
        assert statuses == {lm.OK, lm.NOT_FINITE, lm.TOO_SHORT, lm.SILENT, lm.RATE_REFUSED}
        # without the optional outputs, and without a target: the same records, gain 0
        bare = _run_stage(synth, _spec(target=None, mono=mono), segs, rates, outputs=False)
        for name in ("zbar", "zbar_a", "blocks", "blocks_abs", "blocks_rel", "status"):
            assert np.array_equal(bare["rec"][name], out["rec"][name]), name
        assert not bare["rec"]["gain"].any()
        for a, b in zip(bare["z"], out["z"]):
            assert np.array_equal(a, b, equal_nan=True)


def test_same_pcm_same_bits_wherever_the_segment_lies(synth):
    """(2) a segment alone, and the same PCM as segment 0, 3 and 7 of a batch of other lengths and rates."""
    fs = 11025
    for T in (lm.TILE + 1, 3 * lm.TILE + 77):
        X = lm.signal("dc", 2, T, 77 + T)
        alone = _run_stage(synth, _spec(), [X], [fs])
        lens = [T, 130, 1, T, 0, 9000, 4411, T, 2 * lm.TILE]
        rates = [fs, 8000, 48000, fs, fs, 48000, 8000, fs, 8000]
        segs = [X if j in (0, 3, 7) else lm.signal("noise", 2, n, 31 + j) for j, n in enumerate(lens)]
        got = _run_stage(synth, _spec(), segs, rates)
        again = _run_stage(synth, _spec(), segs, rates)
        assert got["rec"].tobytes() == again["rec"].tobytes()
        for j in (0, 3, 7):
            assert got["rec"][j].tobytes() == alone["rec"][0].tobytes(), (T, j)
            assert np.array_equal(got["z"][j], alone["z"][0]) and np.array_equal(got["y"][j], alone["y"][0])
            assert np.array_equal(got["scaled"][j], alone["scaled"][0])
        assert alone["rec"][0]["status"] == lm.OK


def test_refusals_leave_the_outputs_untouched(synth):
    """(3)"""
    import torch
    from parseoggvorbis_amd import binding
    x = lm.signal("noise", 1, 4000, 1)
    d_pcm = torch.from_numpy(x[None]).cuda()
    d_rec = torch.full((40,), 0xAB, dtype=torch.uint8, device="cuda")
    d_s = torch.full((4000,), float("nan"), dtype=torch.float32, device="cuda")
    bad = [_spec(options=2), _spec(options=0x80000001), _spec(target=float("nan")), _spec(target=0.5), _spec(target=-70.5),
           _spec(target=float("inf")), binding.LoudnessSpec(1, 2, -23.0)]
    for sp in bad:
        with pytest.raises(binding.VsynError) as ei:
            synth.loudness_device(sp, [8000], [4000], d_pcm.data_ptr(), 4000, 1, d_rec.data_ptr(), None, None, 0, d_s.data_ptr(), 4000)
        assert ei.value.code == binding.VSYN_ERR_INVALID
    for kw in (dict(d_records=None), dict(d_pcm=None), dict(plane_stride=0), dict(channels=0), dict(channels=256)):
        a = dict(d_pcm=d_pcm.data_ptr(), plane_stride=4000, channels=1, d_records=d_rec.data_ptr())
        a.update(kw)
        with pytest.raises(binding.VsynError) as ei:
            synth.loudness_device(_spec(), [8000], [4000], a["d_pcm"], a["plane_stride"], a["channels"], a["d_records"])
        assert ei.value.code == binding.VSYN_ERR_INVALID
    with pytest.raises(binding.VsynError):  # a scaled plane without a target
        synth.loudness_device(_spec(target=None), [8000], [4000], d_pcm.data_ptr(), 4000, 1, d_rec.data_ptr(), None, None, 0, d_s.data_ptr(), 4000)
    torch.cuda.synchronize()
    assert (d_rec.cpu().numpy() == 0xAB).all() and np.isnan(d_s.cpu().numpy()).all()
    # the boundaries of the target are accepted
    for t in (-70.0, 0.0):
        synth.loudness_device(_spec(target=t), [8000], [4000], d_pcm.data_ptr(), 4000, 1, d_rec.data_ptr())
    torch.cuda.synchronize()
    assert d_rec.cpu().numpy().view(binding.LOUDNESS_RECORD_DTYPE)[0]["status"] == lm.OK


# ---- (4) the host forms behind a submit ----
def _cond_device(g, cond, plane, frames):
    """vsyn_pcm_condition_device over mono planes (S, stride) float32 with frames [S]: (S, stride) float32."""
    import torch
    S, stride = plane.shape
    d_in = torch.from_numpy(np.ascontiguousarray(plane)).cuda()
    d_fr = torch.from_numpy(np.asarray(frames, np.uint32)).cuda()
    d_out = torch.zeros((S, stride), dtype=torch.float32, device="cuda")
    g.pcm_condition_device(cond, d_in.data_ptr(), stride, 1, S, d_fr.data_ptr(), d_out.data_ptr(), stride, None,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def _same_records(a, b):
    return all(np.array_equal(a[n], b[n]) for n in ("zbar", "zbar_a", "blocks", "blocks_abs", "blocks_rel", "gain", "status"))


def test_host_forms():
    """(4) vsyn_pcm_loudness_host is the stage alone on the submit's PCM (and on the resampler's); the chain forms with loud = NULL
    are the entries without the argument; with it, the stage alone on the plane the chain has there, the scaled plane handed on to
    conditioning and to the spectral rows; a refused spec leaves the outputs untouched; vsyn_pcm_fetch_host and the next submit are
    bit-identical around all of it."""
    from parseoggvorbis_amd import binding, spectral
    from parseoggvorbis_amd.binding import PcmCond, PcmTrim, Synth, VsynError, VSYN_PCM_F32
    from tests.workloads import fixture_like_spec, synth_batch
    spec = fixture_like_spec(2)
    b1 = synth_batch(spec, streams=3, packets_per_stream=64, pattern="mixed", seed=11)  # at least 8192 frames: four hops at 16 kHz
    b2 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=12)
    S = len(b1["segments"])
    rates = [16000, 8000, 12000][:S]
    gp = Synth(spec, device=0, max_streams=4)
    planar = gp.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"])["pcm"]
    gp.close()
    trim, pre, loud = PcmTrim(256, 64, 40.0), PcmCond(2, 0, 0.97), _spec(mono=True)
    sp = spectral.spectral_spec("log_mel", n_fft=400, hop_length=160, n_mels=40)
    outs = []
    for with_loudness in (False, True):
        g = Synth(spec, device=0, max_streams=4)
        assert g.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"], flags=4)["rc"] == 0  # KEEP_PCM
        f1, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        if with_loudness:
            _, frames, _ = g.pcm_condition_host(PcmCond(0, 0, 0.0), S)
            segs = [planar[s][:, :int(frames[s])] for s in range(S)]
            assert min(lm.num_blocks(r, x.shape[1]) for r, x in zip(rates, segs)) >= 1
            # the terminal: the stage alone, both channel modes, native and resampled
            for mono in (False, True):
                m = _spec(target=None, mono=mono)
                r = g.pcm_loudness_host(m, rates, blocks=True)
                alone = _run_stage(g, m, segs, rates, outputs=False)
                assert r["rc"] == 0 and _same_records(r["records"], alone["rec"]) and (r["records"]["status"] == lm.OK).all()
                assert np.array_equal(r["z"], np.concatenate(alone["z"])) and list(r["seg_blocks"]) == [len(z) for z in alone["z"]]
                assert _same_records(g.pcm_loudness_host(m, rates)["records"], r["records"])  # without the series
            rs, rs_frames = g.pcm_resample_host(rates, 16000)
            r = g.pcm_loudness_host(_spec(target=None), rates, 16000, blocks=True)
            alone = _run_stage(g, _spec(target=None), [rs[s][:, :int(rs_frames[s])] for s in range(S)], [16000] * S, outputs=False)
            assert _same_records(r["records"], alone["rec"]) and np.array_equal(r["z"], np.concatenate(alone["z"]))
            # the chain forms
            for gate, split in ((None, False), (trim, False), (trim, True)):
                for out_rate in (0, 16000):
                    st_rates = [out_rate or x for x in rates]
                    plain = (g.pcm_split_host if split else g.pcm_trim_host)(gate, PcmCond(0, 0, 0.0) if gate is None else None, S, rates, out_rate)
                    off = g.pcm_chain_host(gate, split, None, PcmCond(0, 0, 0.0) if gate is None else None, S, rates, out_rate)
                    assert np.array_equal(off["pcm"], plain["pcm"]) and np.array_equal(off["frames"], plain["frames"])
                    on = g.pcm_chain_host(gate, split, loud, None, S, rates, out_rate)
                    assert np.array_equal(on["frames"], plain["frames"])
                    if gate is not None:
                        assert np.array_equal(on["refs"], plain["refs"])
                        assert np.array_equal(on["counts"], plain["counts"]) if split else np.array_equal(on["bounds"], plain["bounds"])
                    mono_segs = [plain["pcm"][s][None, :int(plain["frames"][s])] for s in range(S)]
                    alone = _run_stage(g, _spec(), mono_segs, st_rates, outputs=True)
                    assert _same_records(on["records"], alone["rec"]), (split, out_rate)
                    for s in range(S):
                        T = int(plain["frames"][s])
                        assert np.array_equal(on["pcm"][s][:T], alone["scaled"][s][0]) and not on["pcm"][s][T:].any()
                        if on["records"][s]["status"] == lm.OK:
                            assert np.array_equal(on["pcm"][s][:T], plain["pcm"][s][:T] * on["records"][s]["gain"])
                    assert (on["records"]["status"] == lm.OK).any()
                    # conditioning behind it reads the scaled plane
                    both = g.pcm_chain_host(gate, split, loud, pre, S, rates, out_rate)
                    assert np.array_equal(both["pcm"], _cond_device(g, pre, on["pcm"], on["frames"])) and _same_records(both["records"], on["records"])
                    # and so do the spectral rows, under every other stage
                    rows_off = g.pcm_chain_spectral_host(gate, split, None, None, sp, None, None, rates, out_rate)
                    rows_plain = (g.pcm_split_spectral_host if split else g.pcm_trim_spectral_host)(gate, None, sp, None, rates, out_rate)
                    assert np.array_equal(rows_off["rows"], rows_plain["rows"]) and np.array_equal(rows_off["seg_rows"], rows_plain["seg_rows"])
                    rows_on = g.pcm_chain_spectral_host(gate, split, loud, None, sp, None, None, rates, out_rate)
                    assert _same_records(rows_on["records"], on["records"]) and np.array_equal(rows_on["seg_rows"], rows_plain["seg_rows"])
                    assert rows_on["rows"].shape == rows_plain["rows"].shape and not np.array_equal(rows_on["rows"], rows_plain["rows"])
            # refusals: nothing is written
            for bad_loud, cond in ((_spec(mono=False), None), (_spec(target=None, mono=True), None), (_spec(target=1.0, mono=True), None),
                                   (_spec(options=3, mono=True), None), (loud, PcmCond(1, 0, 0.0)), (loud, PcmCond(3, 0, 0.97))):
                out = np.full((S, 8), 7.0, np.float32)
                fr, rec = np.full(S, 7, np.uint64), np.full(S, 7, np.uint8).repeat(40).view(binding.LOUDNESS_RECORD_DTYPE)
                err = binding.C.c_char_p()
                rc = g.lib.vsyn_pcm_chain_host(g.h, None, 0, binding.C.byref(bad_loud), None if cond is None else binding.C.byref(cond), S,
                                               binding._ptr(binding._rates(rates)), 0, VSYN_PCM_F32, binding._ptr(out), 8, binding._ptr(fr), None,
                                               None, None, 0, None, None, binding._ptr(rec), binding.C.byref(err))
                assert rc == binding.VSYN_ERR_INVALID and (out == 7.0).all() and (fr == 7).all() and (rec.view(np.uint8) == 7).all()
                with pytest.raises(VsynError) as ei:
                    g.pcm_chain_spectral_host(None, False, bad_loud, cond, sp, None, None, rates)
                assert ei.value.code == binding.VSYN_ERR_INVALID
            with pytest.raises(VsynError):
                g.pcm_loudness_host(_spec(options=2), rates)
        f1b, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        assert np.array_equal(f1, f1b)
        r2 = g.submit_host(b2["packets"], b2["segments"], b2["ys"], b2["residue"], b2["plane_stride"])
        assert r2["rc"] == 0
        outs.append((f1, r2["pcm"], r2["emit_len"]))
        g.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])


# ---- (5) end to end on the fixtures ----
LU = 10.0 / np.log(10.0)  # d(LUFS) per relative change of a mean square


@pytest.fixture(scope="module")
def blobs():
    """The two real fixtures, the mono one re-headed to 16 kHz so that the rates differ within a call, and a synthetic stream."""
    from tests.test_gpu_spectral import _ogg, _rehead
    real = [_ogg("test.stereo44khz"), _ogg("test.mono44khz")]
    return real + [_rehead(real[1], 16000), _ogg("synth_03")]


def _expect(x, fs, mono):
    """The model on the product's own PCM x (C, T), with its tolerance in LU for the integrated value and per block."""
    m = lm.measure(x, fs, mono=mono)
    if m["status"] not in (lm.OK, lm.SILENT):
        return m, 0.0, None
    X = float(np.abs(lm.downmix(x) if mono else x).max())
    assert lm.margins_exceed(m, fs, X)
    Bz, _, Bzbar = lm.block_bounds(m, fs, X)
    with np.errstate(divide="ignore", invalid="ignore"):
        tol_z = np.where(m["z"] > 0, LU * Bz / m["z"], 0.0) * 1.01 + 1e-12
    return m, (LU * Bzbar / m["zbar"] * 1.01 + 1e-12 if m["status"] == lm.OK else 0.0), tol_z


@pytest.mark.parametrize("sr", [None, 16000])
def test_get_loudness_batch_against_the_model(blobs, sr):
    """(5a) against the model on get_pcm_batch's own PCM, native rate and sr = 16000, both channel modes."""
    from parseoggvorbis_amd import loudness, pcm
    pcms = pcm.get_pcm_batch(blobs, sr=sr)
    for channels in ("sum", "mono"):
        res = loudness.get_loudness_batch(blobs, sr=sr, channels=channels, blocks=True, errors="return")
        bare = loudness.get_loudness_batch(blobs, sr=sr, channels=channels, errors="return")
        measured = 0
        for i, ((x, fs), r, r0) in enumerate(zip(pcms, res, bare)):
            m, tol, tol_z = _expect(x, fs, channels == "mono")
            if m["status"] not in (lm.OK, lm.SILENT):
                assert isinstance(r, loudness.LoudnessError) and isinstance(r0, loudness.LoudnessError) and "file %d" % i in str(r)
                assert ("too short" in str(r)) == (m["status"] == lm.TOO_SHORT)
                continue
            L, rate, bl = r
            assert rate == fs and r0 == (L, rate) and bl.dtype == np.float64 and len(bl) == m["blocks"]
            assert abs(L - m["lufs"]) <= tol, (i, L, m["lufs"], tol)
            with np.errstate(divide="ignore", invalid="ignore"):
                want = -0.691 + 10.0 * np.log10(m["z"])
            fin = np.isfinite(want)
            assert np.array_equal(np.isfinite(bl), fin) and (np.abs(bl[fin] - want[fin]) <= tol_z[fin]).all()
            print("get_loudness_batch sr %r %s file %d: %.4f LUFS (model %.4f, tolerance %.2g LU)" % (sr, channels, i, L, m["lufs"], tol))
            measured += 1
        assert measured >= 3
    one = loudness.get_loudness_from_raw_bytes(blobs[0], sr=sr)
    assert one == loudness.get_loudness_batch(blobs[:1], sr=sr)[0]


@pytest.mark.parametrize("stages", [dict(), dict(trim_db=40.0), dict(preemphasis=0.97), dict(trim_db=40.0, preemphasis=0.97, sr=16000)],
                         ids=lambda d: "-".join(d) or "plain")
def test_get_pcm_batch_loudness_normalize(synth, blobs, stages):
    """(5b) against the stage alone and the model on the device's own un-normalised mono plane."""
    from parseoggvorbis_amd import pcm
    from parseoggvorbis_amd.binding import PcmCond
    three = blobs[:3]
    gate = {k: v for k, v in stages.items() if k in ("trim_db", "sr")}
    ti, ti0, L = [], [], []
    plain = pcm.get_pcm_batch(three, mono=True, trim_index=ti0, **gate)
    got = pcm.get_pcm_batch(three, mono=True, loudness_normalize=TARGET, loudness=L, trim_index=ti, **stages)
    assert ti == ti0 and len(L) == 3
    for i, ((x, fs), (y, fs1)) in enumerate(zip(plain, got)):
        assert fs == fs1 and x.shape == y.shape and y.dtype == np.float32
        m, tol, _ = _expect(x[None], fs, False)
        assert m["status"] == lm.OK and abs(L[i] - m["lufs"]) <= tol
        alone = _run_stage(synth, _spec(), [x[None]], [fs])
        rec = alone["rec"][0]
        assert rec["gain"].tobytes() == lm.gain(rec["zbar"], TARGET).tobytes() and L[i] == -0.691 + 10.0 * np.log10(rec["zbar"])
        want = x * rec["gain"]
        if "preemphasis" in stages:
            want = _cond_device(synth, PcmCond(2, 0, float(np.float32(stages["preemphasis"]))), want[None], [len(want)])[0]
        assert np.array_equal(y, want), (stages, i)
        # over the blocks the measurement kept, the normalised plane is at the target, up to float32. (Measured afresh it need not
        # be: the absolute gate does not move with the gain, so a block it cut before can pass it afterwards.)
        after = lm.lufs(float(lm.measure((x * rec["gain"])[None], fs)["z"][m["keep_rel"]].mean()))
        assert abs(after - TARGET) < 1e-5, after
    # off: the bits and the entry points of the call without the arguments
    off = pcm.get_pcm_batch(three, mono=True, loudness_normalize=None, loudness=L, **stages)
    ref = pcm.get_pcm_batch(three, mono=True, **stages)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(off, ref)) and L == [None] * 3


@pytest.mark.parametrize("stages", [dict(), dict(split_db=40.0, sr=16000, delta=1, normalize="mean")], ids=lambda d: "-".join(d) or "plain")
def test_get_spectral_batch_loudness_normalize(blobs, stages):
    """(5c) log_mel against tests/spectral_model.py on the device's own normalised plane, under the gates of test_gpu_spectral.py."""
    from parseoggvorbis_amd import pcm, spectral
    from tests.test_gpu_spectral import assert_matches
    three = blobs[:3]
    kw = dict(kind="log_mel", n_fft=400, hop_length=160, n_mels=40)
    gate = {k: v for k, v in stages.items() if k in ("split_db", "sr")}
    L, L2 = [], []
    planes = pcm.get_pcm_batch(three, mono=True, loudness_normalize=TARGET, loudness=L2, **gate)
    got = spectral.get_spectral_batch(three, loudness_normalize=TARGET, loudness=L, **kw, **stages)
    assert L == L2 and all(v is not None for v in L)
    if "delta" not in stages:
        for i, ((x, fs), rows) in enumerate(zip(planes, got)):
            assert_matches(rows, x[None], fs, kw, "loudness_normalize file %d" % i)
    else:  # the post stage behind it: the rows of the call that gets the normalised plane's rows, then delta / normalize alike
        base = spectral.get_spectral_batch(three, loudness_normalize=TARGET, **kw, **gate)
        for i, ((x, fs), rows) in enumerate(zip(planes, base)):
            assert_matches(rows, x[None], fs, kw, "loudness_normalize + split file %d" % i)
        assert all(a.shape == (b.shape[0], 2 * b.shape[1]) for a, b in zip(got, base))


def test_a_refused_file_fails_alone_by_name(blobs):
    from parseoggvorbis_amd import loudness, pcm
    from tests.test_gpu_spectral import _rehead
    data = [blobs[0], _rehead(blobs[1], 3000), blobs[1], blobs[3]]
    res = loudness.get_loudness_batch(data, errors="return")
    assert isinstance(res[1], loudness.LoudnessError) and "file 1" in str(res[1]) and "4000" in str(res[1])
    assert res[0] == loudness.get_loudness_batch(blobs[:1])[0] and res[2] == loudness.get_loudness_batch(blobs[1:2])[0]
    with pytest.raises(loudness.LoudnessError):
        loudness.get_loudness_batch(data)
    got = pcm.get_pcm_batch(data, mono=True, loudness_normalize=TARGET, errors="return")
    assert isinstance(got[1], pcm.PcmError) and "loudness" in str(got[1]) and isinstance(got[0][0], np.ndarray)
