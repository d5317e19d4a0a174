"""Spectral post-processing on the GPU (vsyn_spectral_post_device, vsyn_pcm_spectral_post_host, ogg_vorbis_spectral_corpus_post,
get_spectral_batch(delta=, normalize=)) against the float64 model of tests/spectral_post_model.py.

Gates of the stage alone (test 1), from the arithmetic the device uses, u = 2^-24:
    X block     bit-identical to the input rows.
    deltas      one float32 FMA chain over `width` float32-rounded coefficients: |d| <= (width + 1) u sum_k |c[k]| |X[f+k]| per
                element (one rounding of each coefficient, `width` roundings of the chain).
    normalised  mu and sigma are float64 sums of the device's own float32 Y, so the model is run on those same Y (the delta error of
                a column with a large mean is a property of the deltas, gated above, not of the normalisation). What remains is the
                one rounding of Z to float32: |d| <= NORM_GATE u max_f |Y - mu| / max(sigma, std_floor) per column.
                gate NORM_GATE = 4.0, 4 x the measured worst ratio; measured 1.000 (the unit roundoff of the final rounding).
End to end (test 3) the gate is the per-kind gate eps of tests/test_gpu_spectral.py pushed through the linear maps plus the stage's
own rounding: delta block eps' = eps sum_k |c_o[k]| + the delta bound above (on the model's rows); mean-normalised 2 eps';
mean_var (2 + |Z|) eps' / max(sigma, std_floor); plus u |Z| for the final rounding. Measured maxima of |d| / gate over the grid:
    no normalisation  log_mel 0.085, mfcc 0.080, mel_db 0.315        mean      log_mel 0.040, mfcc 0.035, mel_db 0.148
    mean_var          log_mel 0.036, mfcc 0.022, mel_db 0.100        given     log_mel 0.039, mfcc 0.020, mel_db 0.035
Stage alone, measured: worst delta |d| / bound 0.481.
"""
import ctypes as C

import numpy as np
import pytest

from tests import spectral_model as sm
from tests import spectral_post_model as pm
from tests.test_gpu_spectral import FILES, GATE, _decode_pcm, _ogg, _rate

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NORM_GATE = 4.0
STD_FLOOR = 1e-5

E2E = [
    dict(kind="log_mel", n_fft=400, hop_length=160, n_mels=40),
    dict(kind="mfcc", n_fft=1024, hop_length=256, n_mels=60, n_mfcc=13),
    dict(kind="mel_db", n_fft=400, hop_length=160, n_mels=40),
]


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
def pcm_by_rate(spec_mod):
    """The product's own PCM per fixture: at each file's rate (None) and resampled on the device to 16 kHz."""
    from parseoggvorbis_amd import pcm
    blobs = [_ogg(n) for n in FILES]
    native = _decode_pcm(blobs)
    low = [y for y, _ in pcm.get_pcm_batch(blobs, sr=16000)]
    return {None: dict(zip(FILES, native)), 16000: dict(zip(FILES, low))}


def _post(order=0, width=9, norm=0, stats=0, floor=STD_FLOOR, mean=None, std=None):
    from parseoggvorbis_amd.binding import SpectralPost
    p = SpectralPost(order, width, norm, stats, floor, None if mean is None else mean.ctypes.data, None if std is None else std.ctypes.data)
    p.keep = (mean, std)  # the spec points into them
    return p


def _run_stage(g, post, x, seg_rows):
    """vsyn_spectral_post_device over rows x (total, D) float32 split as seg_rows: (total, D_out) float32, NaN where nothing was written."""
    import torch
    D = x.shape[1]
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.full((x.shape[0] + 3, D * (1 + post.order)), float("nan"), dtype=torch.float32, device="cuda")
    g.spectral_post_device(post, D, seg_rows, d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.isnan(out[x.shape[0]:]).all()  # nothing written past the rows
    return out[:x.shape[0]]


def _rows(rng, F, D):
    x = (rng.standard_normal((F, D)) * rng.uniform(0.1, 20.0, D) + rng.uniform(-30.0, 30.0, D)).astype(np.float32)
    x[:, 0] = (1e3 + 1e-2 * rng.standard_normal(F)).astype(np.float32)  # large mean, small spread
    x[:, 1] = np.float32(2.5)                                             # constant
    return x


def _delta_bound(x64, width, order):
    """(width + 1) u sum_k |c[k]| |X[f+k]| with the rows' clamping."""
    return (width + 1) * U * pm.delta(np.abs(x64), width, order, coefs=np.abs(pm.delta_coefs(width, order)))


def test_stage_alone_against_the_model(synth):
    """(1) vsyn_spectral_post_device on random rows: deltas within the derived bound, normalised values within NORM_GATE."""
    rng = np.random.default_rng(2024)
    worst_delta, worst_norm = 0.0, 0.0
    for D, order, width in ((4, 2, 9), (13, 2, 9), (80, 2, 9), (128, 1, 5), (256, 2, 9), (80, 1, 65), (13, 2, 3), (256, 0, 9), (4, 0, 9)):
        Fs = [37, 0, width, width + 1, 300, 16, 17, 1000, 2 * width]
        if order == 0:
            Fs += [1, 2]
        else:
            Fs = [F for F in Fs if F == 0 or F >= width]  # (a shorter segment is refused: test_stage_refuses_bad_arguments)
        x = np.concatenate([_rows(rng, F, D) for F in Fs])
        off = np.concatenate([[0], np.cumsum(Fs)])
        Dout = D * (1 + order)
        mean = rng.uniform(-5, 5, Dout).astype(np.float32)
        std = rng.uniform(0.5, 3.0, Dout).astype(np.float32)
        std[1] = 0.0  # below the floor
        y = _run_stage(synth, _post(order, width), x, Fs) if order else x
        for gi, F in enumerate(Fs):  # the deltas
            xs = x[off[gi]:off[gi + 1]]
            ys = y[off[gi]:off[gi + 1]]
            assert np.array_equal(ys[:, :D], xs), (D, order, width, gi)
            for o in range(1, order + 1):
                if F == 0:
                    continue
                want = pm.delta(xs, width, o)
                bound = _delta_bound(xs.astype(np.float64), width, o)
                d = np.abs(ys[:, o * D:(o + 1) * D].astype(np.float64) - want)
                assert (d <= bound).all(), (D, o, width, gi, float((d / np.maximum(bound, 1e-300)).max()))
                worst_delta = max(worst_delta, float((d / np.maximum(bound, 1e-300)).max()))
        for norm, stats in ((1, 0), (2, 0), (1, 1), (2, 1)):
            post = _post(order, width, norm, stats, STD_FLOOR, mean, std if norm == 2 else None)
            z = _run_stage(synth, post, x, Fs)
            for gi, F in enumerate(Fs):
                if F == 0:
                    continue
                ys = y[off[gi]:off[gi + 1]].astype(np.float64)
                given = (mean, std if norm == 2 else None) if stats else None
                want = pm.normalize(ys, "mean" if norm == 1 else "mean_var", given=given, std_floor=STD_FLOOR)
                mu, sigma = (mean.astype(np.float64), std.astype(np.float64)) if stats else pm.stats(ys)
                den = np.maximum(sigma, STD_FLOOR) if norm == 2 else 1.0
                scale = np.abs(ys - mu).max(axis=0) / den
                d = np.abs(z[off[gi]:off[gi + 1]].astype(np.float64) - want)
                assert (d <= NORM_GATE * U * scale).all(), (D, order, width, norm, stats, gi, float((d / np.maximum(U * scale, 1e-300)).max()))
                nz = scale > 0
                if nz.any():
                    worst_norm = max(worst_norm, float((d[:, nz] / (U * scale[nz])).max()))
                if not stats:  # the constant column becomes zeros
                    assert (z[off[gi]:off[gi + 1], 1] == 0).all()
    print("stage alone: worst delta |d| / bound %.3f, worst normalised ratio %.3f (gate %.1f)" % (worst_delta, worst_norm, NORM_GATE))


def test_stage_refuses_bad_arguments(synth):
    from parseoggvorbis_amd.binding import VsynError
    x = np.zeros((20, 8), np.float32)
    for post, rows in ((_post(1, 9), [12, 8]), (_post(3, 9), [20]), (_post(1, 4), [20]), (_post(0, 9, 2, 0, 0.0), [20]),
                       (_post(0, 9, 2, 1), [20]), (_post(0, 9, 1, 1, STD_FLOOR, np.full(8, np.nan, np.float32)), [20])):
        with pytest.raises(VsynError) as ei:
            _run_stage(synth, post, x, rows)
        assert ei.value.code == 1, str(ei.value)  # VSYN_ERR_INVALID
    with pytest.raises(VsynError) as ei:
        _run_stage(synth, _post(2, 9), x, [12, 8])
    assert "segment 1" in str(ei.value) and "width 9" in str(ei.value) and "has 8" in str(ei.value)


def test_same_bits_twice_and_wherever_the_segment_lies(synth):
    """(2) a segment alone and as the third of five gives the same bits; two runs give the same bits."""
    rng = np.random.default_rng(7)
    for D, order, width, norm in ((80, 2, 9, 2), (13, 2, 9, 2), (4, 1, 5, 1), (256, 2, 9, 2), (80, 0, 9, 2)):
        Fs = [50, 300, 777, 9, 1203]
        segs = [_rows(rng, F, D) for F in Fs]
        post = _post(order, width, norm)
        alone = _run_stage(synth, post, segs[2], [Fs[2]])
        both = _run_stage(synth, post, np.concatenate(segs), Fs)
        again = _run_stage(synth, post, np.concatenate(segs), Fs)
        assert np.array_equal(both, again), (D, order)
        o = Fs[0] + Fs[1]
        assert np.array_equal(both[o:o + Fs[2]], alone), (D, order)
        assert not np.isnan(both).any()


def _given(dout, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-3.0, 3.0, dout).astype(np.float32), rng.uniform(0.5, 4.0, dout).astype(np.float32)


def _compare_batch(spec_mod, pcm, kw, delta, width, normalize, sr, hop_note=""):
    """One get_spectral_batch call over FILES with errors="return": the failed files are exactly those the model predicts from F
    (0 < F < width), each message names the width and the frame count, every other file is within the gate. Returns (compared, worst
    |d| / gate)."""
    datas = [_ogg(n) for n in FILES]
    res = spec_mod.get_spectral_batch(datas, errors="return", sr=sr, delta=delta, delta_width=width, normalize=normalize,
                                      std_floor=STD_FLOOR, **kw)
    compared, worst = 0, 0.0
    eps = GATE[kw["kind"]]
    for name, data, got in zip(FILES, datas, res):
        x = pcm[sr][name]
        rate = sr or _rate(data)
        F = sm.num_frames(x.shape[1], kw["n_fft"], kw["hop_length"], True)
        if 0 < F < width:
            assert isinstance(got, spec_mod.SpectralError), (name, F)
            assert "width %d" % width in str(got) and "has %d" % F in str(got), str(got)
            continue
        assert isinstance(got, np.ndarray), (name, F, got)
        base, _ = sm.spectral(x, rate, **kw)
        D = base.shape[1]
        assert got.shape == (F, D * (1 + delta)) and got.dtype == np.float32, (name, got.shape)
        if F == 0:
            continue
        y = pm.with_deltas(base, delta, width)
        epsb = np.full(y.shape, eps)  # eps' per element: the bound of the column's block
        for o in range(1, delta + 1):
            epsb[:, o * D:(o + 1) * D] = eps * np.abs(pm.delta_coefs(width, o)).sum() + _delta_bound(base, width, o)
        if normalize is None:
            want, tol = y, epsb
        else:
            want = pm.post(base, delta, width, normalize, STD_FLOOR)
            epsc = epsb.max(axis=0)
            if normalize == "mean" or (isinstance(normalize, tuple) and normalize[1] is None):
                tol = 2.0 * epsc + U * np.abs(want)
            else:
                sigma = pm.stats(y)[1] if normalize == "mean_var" else np.asarray(normalize[1], np.float64)
                tol = (2.0 + np.abs(want)) * epsc / np.maximum(sigma, STD_FLOOR) + U * np.abs(want)
        d = np.abs(got.astype(np.float64) - want)
        ratio = float((d / tol).max())
        assert (d <= tol).all(), (name, kw, delta, normalize if not isinstance(normalize, tuple) else "given", sr, hop_note, ratio)
        worst = max(worst, ratio)
        compared += 1
    return compared, worst


def test_end_to_end_against_the_models(spec_mod, pcm_by_rate):
    """(3) get_spectral_batch over every fixture, E2E x delta x normalize x sr, against spectral_model then the post model."""
    worst = {}
    for kw in E2E:
        dim = kw.get("n_mfcc", kw["n_mels"]) if kw["kind"] == "mfcc" else kw["n_mels"]
        for delta in (1, 2):
            mean, std = _given(dim * (1 + delta), delta)
            for label, normalize in (("none", None), ("mean", "mean"), ("mean_var", "mean_var"), ("given", (mean, std))):
                for sr in (None, 16000):
                    n, w = _compare_batch(spec_mod, pcm_by_rate, kw, delta, 9, normalize, sr)
                    assert n > 0, (kw, delta, label, sr, n)  # (which files are short is the model's word, checked per file)
                    key = (kw["kind"], label)
                    worst[key] = max(worst.get(key, 0.0), w)
    print("end to end, worst |d| / gate:", {"%s/%s" % k: round(v, 4) for k, v in sorted(worst.items())})


def test_short_files_fail_alone_and_only_they(spec_mod, pcm_by_rate):
    """(4) 0 < F < width fails that file by name and no other: width 9 at hop 160 leaves at least 15 of the 19 fixtures, width 3 all."""
    kw = dict(kind="log_mel", n_fft=400, hop_length=160, n_mels=40)
    counts = {}
    for width in (9, 5, 3):
        counts[width], _ = _compare_batch(spec_mod, pcm_by_rate, kw, 1, width, "mean_var", None)
    assert counts[9] >= 15 and counts[5] >= counts[9] and counts[3] == len(FILES) == 19, counts
    assert counts[9] < 19  # the grid does contain short files
    # the boundary: hop 441 leaves fixtures at 8 - 10 frames, on either side of width 9 (not counted above)
    n, _ = _compare_batch(spec_mod, pcm_by_rate, dict(kind="log_mel", n_fft=1102, hop_length=441, n_mels=80), 2, 9, "mean", None, "hop 441")
    assert n >= 1
    # errors="raise" names the first short file
    with pytest.raises(spec_mod.SpectralError) as ei:
        spec_mod.get_spectral_batch([_ogg(n) for n in FILES], delta=1, **kw)
    assert "width 9" in str(ei.value) and "file " in str(ei.value)


def test_off_means_off(spec_mod, synth):
    """(5) delta=0, normalize=None is the call without the keywords, bit for bit; a post spec that is off gives the bits of
    vsyn_pcm_spectral_host; a post call leaves vsyn_pcm_fetch_host and the next submit alone."""
    from parseoggvorbis_amd.binding import Synth, VSYN_PCM_F32
    from tests.workloads import fixture_like_spec, synth_batch
    datas = [_ogg(n) for n in FILES]
    for kw in (E2E[0], E2E[1]):
        a = spec_mod.get_spectral_batch(datas, **kw)
        b = spec_mod.get_spectral_batch(datas, delta=0, delta_width=5, normalize=None, std_floor=1.0, **kw)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
    spec = fixture_like_spec(2)
    b1 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=11)
    b2 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=12)
    S = len(b1["segments"])
    outs = []
    for with_post in (False, True):
        g = Synth(spec, device=0, max_streams=4)
        r1 = g.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"], flags=4)  # KEEP_PCM
        assert r1["rc"] == 0
        f1, fr1 = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        if with_post:
            for kw in (dict(kind="mfcc"), dict(kind="log_mel", n_fft=400, hop_length=160, n_mels=40)):
                s = spec_mod.spectral_spec(**kw)
                plain = g.pcm_spectral_host(s, [44100] * S)
                off = g.pcm_spectral_post_host(s, _post(0, 9, 0), [44100] * S)
                assert np.array_equal(off["rows"], plain["rows"]) and np.array_equal(off["seg_rows"], plain["seg_rows"])
                for out_rate in (0, 16000):
                    # (resampled to 16 kHz the segments have 3 mfcc frames: width 3 there)
                    r = g.pcm_spectral_post_host(s, _post(2, 3 if out_rate else 9, 2), [44100] * S, out_rate)
                    assert r["rc"] == 0 and r["rows"].shape == (int(r["seg_rows"].sum()), 3 * plain["rows"].shape[1])
                    if out_rate:
                        continue
                    o = 0
                    for gi in range(S):  # each segment: the model's stage over the rows of the plain call
                        nr = int(r["seg_rows"][gi])
                        base = plain["rows"][o:o + nr].astype(np.float64)
                        want = pm.post(base, 2, 9, "mean_var", STD_FLOOR)
                        bound = np.concatenate([np.zeros_like(base)] + [_delta_bound(base, 9, k) for k in (1, 2)], axis=1)
                        sigma = pm.stats(pm.with_deltas(base, 2, 9))[1]
                        tol = (2.0 + np.abs(want)) * bound.max(axis=0) / np.maximum(sigma, STD_FLOOR) + NORM_GATE * U * np.abs(want).max(axis=0)
                        assert (np.abs(r["rows"][o:o + nr] - want) <= tol).all(), (kw, gi)
                        o += nr
        f1b, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        assert np.array_equal(f1, f1b)
        r2 = g.submit_host(b2["packets"], b2["segments"], b2["ys"], b2["residue"], b2["plane_stride"])
        assert r2["rc"] == 0
        outs.append((f1, r2["pcm"], r2["emit_len"]))
        g.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])


def test_a_damaged_file_fails_alone_with_the_stage_on(spec_mod):
    """(6) one corrupt file in a replicated corpus: it fails with its own error, every other file equals its single-file result."""
    names = ["test.stereo44khz", "synth_02", "test.mono44khz", "synth_10"] * 3
    blobs = [_ogg(n) for n in names]
    bad = bytearray(blobs[5])
    bad[len(bad) // 2] ^= 0x55  # a page CRC
    blobs[5] = bytes(bad)
    kw = dict(kind="log_mel", n_fft=256, hop_length=64, n_mels=64, delta=2, normalize="mean_var")
    res = spec_mod.get_spectral_batch(blobs, errors="return", files_per_submit=4, **kw)
    single = {n: spec_mod.get_spectral_from_raw_bytes(_ogg(n), **kw) for n in set(names)}
    assert all(isinstance(v, np.ndarray) and v.shape[0] >= 9 and v.shape[1] == 192 for v in single.values())  # all four have F >= width
    for i, (n, r) in enumerate(zip(names, res)):
        if i == 5:
            assert isinstance(r, spec_mod.SpectralError) and "file 5" in str(r)
            continue
        assert isinstance(r, np.ndarray), (i, r)
        assert np.array_equal(r, single[n]), i
