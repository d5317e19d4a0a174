"""The inverse STFT on the GPU (include/vorbis_synth_hip.h, "inverse STFT"): every sample of every case against the float64 model
under the derived per-sample bound of tests/istft_model.py. No sample is excluded: one with a small window-sum-square has a wide
bound, not an exemption. Each case prints its worst |d| / bound; DESIGN.md 6q has the table.

Measured on the MI355X (worst |d| / bound, plain / masked): 16 / 7 0.056 / 0.054, 1024 / 256 / 700 0.005 / 0.005, 2048 / 512 0.003 /
0.003, 8192 / 2048 0.001 / 0.002, 64 / 1 uncentred 0.019 / 0.022, 512 / 700 / 400 0.011 / 0.013; round trip at most 0.012."""
import ctypes as C

import numpy as np
import pytest

from tests import istft_model as im
from tests import spectral_lin_model as lm
from tests import spectral_model as sm
from tests.test_gpu_spectral_lin import mono_batch, run_device

pytestmark = pytest.mark.gpu

TAIL = 19  # NaN sentinels behind the longest output


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


def raw_spec(n_fft, hop, win, center=True):
    """A vsyn_spectral_spec without the Python-side checks: what a C caller may pass."""
    from parseoggvorbis_amd.binding import SpectralSpec
    return SpectralSpec(kind=7, options=1 if center else 0, n_fft=n_fft, hop_length=hop, win_length=win)


def run_istft(g, spec, rows, masks, lengths, plane=None):
    """vsyn_istft_device on a batch: rows (list of complex64 [F_g][NB]), masks (a list of float32 [F_g][NB], or None), lengths (a
    list, or None). Returns each segment's samples (float32 [length_g]). The output planes start as NaN: everything behind a
    segment's length must still be NaN, the inputs unchanged, and d_out_frames the lengths."""
    import torch
    n = spec.n_fft
    nb = n // 2 + 1
    S = len(rows)
    center = bool(spec.options & 1)
    lens = [im.num_samples(r.shape[0], n, spec.hop_length, center) for r in rows] if lengths is None else list(lengths)
    plane = max(lens + [1]) + TAIL if plane is None else plane
    flat = np.concatenate([np.asarray(r, np.complex64).reshape(-1, nb) for r in rows] + [np.zeros((1, nb), np.complex64)])
    d_rows = torch.from_numpy(flat.view(np.float32).copy()).cuda()
    d_mask = None
    if masks is not None:
        mflat = np.concatenate([np.asarray(m, np.float32).reshape(-1, nb) for m in masks] + [np.zeros((1, nb), np.float32)])
        d_mask = torch.from_numpy(mflat.copy()).cuda()
    d_out = torch.full((S, plane), float("nan"), dtype=torch.float32, device="cuda")
    d_frames = torch.full((S + 1,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    g.istft_device(spec, [r.shape[0] for r in rows], d_rows.data_ptr(), None if d_mask is None else d_mask.data_ptr(), lengths, d_out.data_ptr(),
                   plane, d_frames.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out, fr = d_out.cpu().numpy(), d_frames.cpu().numpy()
    assert np.array_equal(d_rows.cpu().numpy().view(np.uint32), flat.view(np.uint32))  # read only
    if d_mask is not None:
        assert np.array_equal(d_mask.cpu().numpy().view(np.uint32), mflat.view(np.uint32))
    assert list(fr[:S]) == lens and fr[S] == 0x7FFFFFFF
    for s in range(S):
        assert np.isnan(out[s, lens[s]:]).all(), ("sentinels", s)
    return [out[s, :lens[s]].copy() for s in range(S)]


def tile_of(g, spec_mod, n):
    return g.lib.vsyn_spectral_lin_tile(C.byref(spec_mod.spectral_spec("stft", n_fft=n, hop_length=max(n // 4, 1))))


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("entry", im.FRAMINGS, ids=im.fid)
def test_stage_against_the_model(spec_mod, synth, entry, masked):
    """Ten segments a call, random complex rows (no valid STFT), row counts around the tile, lengths equal to, shorter than and
    longer than what the frames cover."""
    n, hop, win, center = entry
    tile = tile_of(synth, spec_mod, n)
    counts = [0, 1, 2, 3, 5, 0, 1, 2, 3, 5] if n == 8192 else [0, 1, 2, tile - 1, tile, tile + 1, 33, 130, 7, 2 * tile + 1]
    rng = np.random.default_rng(n + 7 * masked)
    rows = [im.random_rows(rng, F, n) for F in counts]
    masks = [rng.random(r.shape).astype(np.float32) for r in rows] if masked else None
    cover = [im.num_samples(F, n, hop, center) for F in counts]
    lengths = [max(c + (0, -min(c, n // 3 + 1), 37)[i % 3], 0) for i, c in enumerate(cover)]
    assert any(l < c for l, c in zip(lengths, cover)) and any(l > c for l, c in zip(lengths, cover))
    spec = raw_spec(n, hop, win, center)
    got = run_istft(synth, spec, rows, masks, lengths)
    worst = 0.0
    for s, F in enumerate(counts):
        worst = max(worst, im.check(got[s], rows[s], n, hop, win, center, lengths[s], None if masks is None else masks[s], what=(entry, masked, s, F)))
        if F == 0:
            assert not got[s].any()
    print("istft %s %s: worst |d| / bound %.3f" % (im.fid(entry), "masked" if masked else "plain", worst))
    assert worst > 0.0
    # lengths = NULL: what the rows cover
    dflt = run_istft(synth, spec, rows[:4], None if masks is None else masks[:4], None)
    for s in range(4):
        assert dflt[s].shape[0] == cover[s] == synth.lib.vsyn_istft_num_samples(C.byref(spec), counts[s])
        k = min(cover[s], lengths[s])
        assert np.array_equal(dflt[s][:k].view(np.uint32), got[s][:k].view(np.uint32))


@pytest.mark.parametrize("entry", im.FRAMINGS[:4], ids=im.fid)
def test_round_trip(spec_mod, synth, entry):
    """The stft kind on noise, a sine plus 1e-4 noise, and a loud burst beside near-silence, then the inverse to length T: the
    signal again, gated by the inverse's bound (on the device's own rows) plus the forward bound carried through the model inverse:
    each component of a bin is within B_f, so x_f[j] moves by at most 2 B_f, weighted by w and divided by W like the signal."""
    n, hop, win, center = entry
    T = hop * 9 + hop // 3 if n == 8192 else hop * 40 + hop // 3
    sig = lm.signals(T, n)
    names = ["noise", "sine", "burst"]
    pcm, frames = mono_batch([sig[k] for k in names])
    fwd = spec_mod.spectral_spec("stft", n_fft=n, hop_length=hop, win_length=win, center=center)
    rows = [r.view(np.complex64) for r in run_device(synth, fwd, pcm, frames, [44100] * len(names))]
    got = run_istft(synth, raw_spec(n, hop, win, center), rows, None, [T] * len(names))
    w = lm.window32(n, win).astype(np.float64)
    worst = 0.0
    for name, X, y in zip(names, rows, got):
        B = lm.stft(sig[name], n, hop, win, center)[1]
        carried = im.overlap_add(np.zeros((X.shape[0], n)), w, n, hop, win, center, T, dv=w[None, :] * 2.0 * B[:, None])[3]
        ym, b = im.istft(X, n, hop, win, center, T)
        tol = b + carried * (1.0 + 2.0 ** -40) + 1e-13
        d = np.abs(y.astype(np.float64) - sig[name].astype(np.float64))
        assert (d <= tol).all(), (entry, name, float((d / tol).max()))
        worst = max(worst, float((d / tol).max()))
    print("round trip %s: worst |d| / (forward + inverse bound) %.3f" % (im.fid(entry), worst))


@pytest.mark.parametrize("entry", [im.FRAMINGS[0], im.FRAMINGS[1], im.FRAMINGS[5]], ids=im.fid)
def test_same_rows_same_bits(spec_mod, synth, entry):
    """A segment alone, and as segment 0, 3 or 7 of a batch of ten whose other rows and masks are full of 1e30."""
    n, hop, win, center = entry
    rng = np.random.default_rng(n)
    F = 2 * tile_of(synth, spec_mod, n) + 1
    X, m = im.random_rows(rng, F, n), rng.random((F, n // 2 + 1)).astype(np.float32)
    spec = raw_spec(n, hop, win, center)
    L = im.num_samples(F, n, hop, center) + 11
    alone = run_istft(synth, spec, [X], [m], [L])[0]
    assert np.isfinite(alone).all() and alone.any()
    for pos in (0, 3, 7):
        counts = [5, 0, 3, 1, 9, 2, 4, 6, 1, 3]
        rows = [np.full((c, n // 2 + 1), 1e30 + 1e30j, np.complex64) for c in counts]
        masks = [np.full((c, n // 2 + 1), 1e30, np.float32) for c in counts]
        rows[pos], masks[pos] = X, m
        lens = [im.num_samples(r.shape[0], n, hop, center) for r in rows]
        lens[pos] = L
        got = run_istft(synth, spec, rows, masks, lens)[pos]
        assert np.array_equal(got.view(np.uint32), alone.view(np.uint32)), (entry, pos)


@pytest.mark.parametrize("entry", [im.FRAMINGS[0], im.FRAMINGS[1], im.FRAMINGS[2]], ids=im.fid)
def test_nonfinite_footprint(spec_mod, synth, entry):
    """A NaN or an Inf in one bin of row f, or in its mask, at f = 0, F - 1 and both sides of a tile edge: exactly the samples
    under frame f's window support are non-finite; every other sample of every segment is bit-equal to the clean run."""
    n, hop, win, center = entry
    tile = tile_of(synth, spec_mod, n)
    rng = np.random.default_rng(n + 1)
    F = 3 * tile + 2
    nb = n // 2 + 1
    rows = [im.random_rows(rng, c, n) for c in (4, F, 3)]
    masks = [rng.random(r.shape).astype(np.float32) for r in rows]
    spec = raw_spec(n, hop, win, center)
    L = im.num_samples(F, n, hop, center) + 5
    lens = [None, L, None]
    lens = [im.num_samples(r.shape[0], n, hop, center) if l is None else l for r, l in zip(rows, lens)]
    clean = run_istft(synth, spec, rows, masks, lens)
    assert all(np.isfinite(c).all() for c in clean)
    woff, pad = (n - win) // 2, (n // 2 if center else 0)
    cases = [(0, 1, np.nan, False), (F - 1, nb - 1, np.inf, False), (tile - 1, 0, -np.inf, False), (tile, nb // 2, np.nan, True),
             (2 * tile, 3, np.inf, True)]
    for f, k, val, in_mask in cases:
        r2, m2 = [r.copy() for r in rows], [m.copy() for m in masks]
        if in_mask:
            m2[1][f, k] = val
        else:
            r2[1][f, k] = complex(val, rows[1][f, k].imag)
        got = run_istft(synth, spec, r2, m2, lens)
        j = np.arange(L) + pad - f * hop
        under = (j >= woff) & (j < woff + win)
        assert under.any() and not np.isfinite(got[1][under]).any(), (entry, f, k, val)
        assert np.array_equal(got[1][~under].view(np.uint32), clean[1][~under].view(np.uint32)), (entry, f, k, val)
        for s in (0, 2):
            assert np.array_equal(got[s].view(np.uint32), clean[s].view(np.uint32))
    # the imaginary parts of the two end bins are not read
    r2 = [r.copy() for r in rows]
    r2[1][1, 0] = complex(rows[1][1, 0].real, np.nan)
    r2[1][1, nb - 1] = complex(rows[1][1, nb - 1].real, np.inf)
    got = run_istft(synth, spec, r2, masks, lens)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, clean))


def test_refusals_leave_the_outputs_untouched(spec_mod, synth):
    import torch
    from parseoggvorbis_amd.binding import VsynError
    n, hop, win = 64, 16, 64
    nb = n // 2 + 1
    F = 5
    L = im.num_samples(F, n, hop, True)
    d_rows = torch.ones((F, nb, 2), dtype=torch.float32, device="cuda")
    d_out = torch.full((L + 3,), float("nan"), dtype=torch.float32, device="cuda")
    d_frames = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(spec, rows=d_rows.data_ptr(), out=d_out.data_ptr(), plane=L + 3, lengths=(L,), seg_rows=(F,)):
        synth.istft_device(spec, seg_rows, rows, None, lengths, out, plane, d_frames.data_ptr(), stream)

    good = raw_spec(n, hop, win)
    refused = [
        ("power of two", lambda: call(raw_spec(1102, 441, 1102))),
        ("n_fft", lambda: call(raw_spec(8, 2, 8))),
        ("n_fft", lambda: call(raw_spec(16384, 4096, 16384))),
        ("hop_length", lambda: call(raw_spec(n, 0, win))),
        ("win_length", lambda: call(raw_spec(n, hop, n + 1))),
        ("NULL", lambda: call(good, rows=None)),
        ("NULL", lambda: call(good, out=None)),
        ("out_plane_stride", lambda: call(good, plane=L - 1)),
    ]
    for word, fn in refused:
        with pytest.raises(VsynError) as e:
            fn()
        assert word in str(e.value), (word, str(e.value))
    err = C.c_char_p()
    lens = np.array([L], np.uint64)
    rc = synth.lib.vsyn_istft_device(synth.h, C.byref(good), 1, None, d_rows.data_ptr(), None, C.c_void_p(lens.ctypes.data), d_out.data_ptr(), L + 3,
                                     None, stream, C.byref(err))
    assert rc != 0 and b"seg_rows" in err.value
    assert synth.lib.vsyn_istft_device(synth.h, None, 0, None, None, None, None, None, 0, None, stream, C.byref(err)) != 0
    assert synth.lib.vsyn_istft_num_samples(C.byref(raw_spec(1102, 441, 1102)), 9) == 0
    torch.cuda.synchronize()
    assert np.isnan(d_out.cpu().numpy()).all() and int(d_frames.cpu()[0]) == 77
    call(good)  # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.isfinite(out[:L]).all() and np.isnan(out[L:]).all() and int(d_frames.cpu()[0]) == L
