"""Linear spectra (include/vorbis_synth_hip.h, "linear spectra"): what needs no GPU — the kinds' encoding and dim on both sides of
the C ABI, the refusal of the post stage before the library loads, the float64 model (tests/spectral_lin_model.py) against the
matrix-product DFT of tests/spectral_model.py, and a float32 numpy restatement of the device's FFT order inside the per-frame
bound on every input of the GPU grid (so that the bound is neither vacuous nor too tight before any GPU run)."""
import ctypes

import numpy as np
import pytest

from parseoggvorbis_amd import spectral
from tests import spectral_lin_model as lm
from tests import spectral_model as sm


def test_the_linear_kinds_encode_5_6_7():
    assert [spectral.spectral_spec(k).kind for k in ("lin_power", "lin_db", "stft")] == [5, 6, 7]
    s = spectral.spectral_spec("lin_db", n_fft=1024, hop_length=256, power=1, amin=1e-5, top_db=None)
    assert (s.kind, s.n_fft, s.hop_length, s.win_length, s.power, s.amin, s.top_db) == (6, 1024, 256, 1024, 1, 1e-5, 0.0)
    from parseoggvorbis_amd import binding
    assert (binding.VSYN_SPEC_LIN_POWER, binding.VSYN_SPEC_LIN_DB, binding.VSYN_SPEC_STFT) == (5, 6, 7)


@pytest.mark.parametrize("n_fft", [16, 1102, 8192])
def test_spec_dim_of_the_linear_kinds(n_fft):
    nb = n_fft // 2 + 1
    dims = [spectral.spec_dim(spectral.spectral_spec(k, n_fft=n_fft, hop_length=4)) for k in ("lin_power", "lin_db", "stft")]
    assert dims == [nb, nb, 2 * nb]


def test_library_dim_agrees_for_every_kind():
    from parseoggvorbis_amd import binding
    lib = binding.load()
    assert "vsyn_spectral_dim" in binding.declared_symbols() and lib.vsyn_abi_version() == 5
    for kind, code in spectral.KINDS.items():
        for n_fft in (16, 1102, 8192):
            s = spectral.spectral_spec(kind, n_fft=n_fft, hop_length=4, n_mels=40, n_mfcc=13)
            assert s.kind == code
            assert lib.vsyn_spectral_dim(ctypes.byref(s)) == spectral.spec_dim(s) > 0, (kind, n_fft)
    assert sorted(spectral.KINDS.values()) == [1, 2, 3, 4, 5, 6, 7]
    for bad in (0, 8):
        s = spectral.spectral_spec()
        s.kind = bad
        assert lib.vsyn_spectral_dim(ctypes.byref(s)) == 0 and spectral.spec_dim(s) == 0
    # a linear kind reads no mel field: garbage there is neither refused nor read
    s = spectral.spectral_spec("stft", n_fft=64, hop_length=8)
    s.n_mels, s.n_mfcc, s.fmin, s.fmax, s.log_floor, s.power, s.amin = 0, 999, -5.0, 1.0, -1.0, 7, -1.0
    assert lib.vsyn_spectral_dim(ctypes.byref(s)) == 66
    s.kind = 5
    assert lib.vsyn_spectral_dim(ctypes.byref(s)) == 0  # lin_power reads power
    s.power = 1
    assert lib.vsyn_spectral_dim(ctypes.byref(s)) == 33


def test_library_frame_count_accepts_the_linear_kinds():
    from parseoggvorbis_amd import binding
    lib = binding.load()
    for kind in ("lin_power", "lin_db", "stft"):
        for kw in (dict(n_fft=1102, hop_length=441), dict(n_fft=16, hop_length=3, center=False), dict(n_fft=8192, hop_length=2048)):
            s = spectral.spectral_spec(kind, **kw)
            for T in (0, 1, 15, 16, 1101, 1102, 8191, 8192, 44100):
                want = sm.num_frames(T, s.n_fft, s.hop_length, bool(s.options & spectral.OPT_CENTER))
                assert lib.vsyn_spectral_num_frames(ctypes.byref(s), T) == want, (kind, kw, T)


def test_library_refuses_the_post_stage_for_a_linear_kind():
    from parseoggvorbis_amd import binding
    lib = binding.load()
    on, _, _ = spectral.post_spec(33, delta=1)
    off = binding.SpectralPost(0, 9, 0, 0, 1e-5, None, None)
    for kind in ("lin_power", "lin_db", "stft"):
        s = spectral.spectral_spec(kind, n_fft=64, hop_length=8)
        assert lib.vsyn_spectral_post_dim(ctypes.byref(s), ctypes.byref(on)) == 0
        assert lib.vsyn_spectral_post_dim(ctypes.byref(s), ctypes.byref(off)) == spectral.spec_dim(s)
    s = spectral.spectral_spec("mel_power", n_mels=33)
    assert lib.vsyn_spectral_post_dim(ctypes.byref(s), ctypes.byref(on)) == 66


@pytest.mark.parametrize("kind", ["lin_power", "lin_db", "stft"])
@pytest.mark.parametrize("kw", [dict(delta=1), dict(delta=2), dict(normalize="mean"), dict(normalize="mean_var")])
def test_delta_and_normalize_raise_before_the_library_loads(kind, kw, monkeypatch):
    def no_load():
        raise AssertionError("library loaded before the arguments were checked")
    monkeypatch.setattr(spectral, "_load", no_load)
    with pytest.raises(spectral.SpectralError) as ei:
        spectral.get_spectral_batch([b"OggS"], kind=kind, n_fft=64, hop_length=16, **kw)
    assert kind in str(ei.value)
    with pytest.raises(spectral.SpectralError):
        spectral.get_spectral_from_raw_bytes(b"OggS", kind=kind, **kw)


@pytest.mark.parametrize("n_fft,hop,win", [(64, 16, 64), (1102, 441, 1102), (64, 16, 40)])
def test_model_equals_the_matrix_product_dft(n_fft, hop, win):
    x = (0.3 * np.random.default_rng(n_fft).standard_normal((2, 5000))).astype(np.float32)
    X, B = lm.stft(x, n_fft, hop, win)
    # sm.spectrum uses the float64 window, the model the float32-rounded one
    w64, w32 = sm.window(n_fft, win), lm.window32(n_fft, win).astype(np.float64)
    S = sm.spectrum(x, n_fft, hop, win, True, 2.0)
    assert X.shape == S.shape == (sm.num_frames(5000, n_fft, hop), n_fft // 2 + 1) and B.shape == (X.shape[0],)
    # |X32|^2 against |X64|^2: the windows differ by at most u per tap, so the spectra by at most u * sum |w y| per component
    A = np.abs(lm.frames(x, n_fft, hop, win)[0]).sum(axis=1)[:, None]
    assert np.abs(w64 - w32).max() <= lm.U
    assert (np.abs(np.abs(X) - np.sqrt(S)) <= 2.0 * lm.U * A + 1e-9 * np.sqrt(S).max()).all()
    # and exactly (1e-9 relative) when the matrix product is given the same rounded window
    v = lm.frames(x, n_fft, hop, win)[0]
    jk = np.outer(np.arange(n_fft), np.arange(n_fft // 2 + 1)) % n_fft
    ang = 2.0 * np.pi * jk / n_fft
    Xm = v @ np.cos(ang) - 1j * (v @ np.sin(ang))
    assert np.abs(Xm - X).max() <= 1e-9 * np.abs(X).max()


@pytest.mark.parametrize("n_fft", [16, 64, 512, 2048, 8192])
def test_float32_restatement_of_the_device_fft_is_within_the_bound(n_fft):
    entries = [g for g in lm.GRID if g[0] == n_fft] + [(n_fft, max(n_fft // 4, 1), n_fft, True, min(20000, 6 * n_fft + 37))]
    worst = 0.0
    for (n, hop, win, center, T) in entries:
        sig = lm.signals(T, n)
        # the impulses of the GPU test as well: a unit impulse at every position of a frame (hop 1 over one impulse)
        if n <= 64:
            imp = np.zeros(3 * n, np.float32)
            imp[2 * n - 1] = 1.0
            sig["impulse"] = imp
        for name, y in sig.items():
            h, c = (1, False) if name == "impulse" else (hop, center)
            X, B = lm.stft(y, n, h, win, c)
            v32 = (lm.window32(n, win)[None, :] * _frame_samples(y, n, h, c)).astype(np.float32)
            re, im = lm.fft_f32(v32, n)
            d = np.maximum(np.abs(re - X.real), np.abs(im - X.imag))
            assert (d <= B[:, None]).all(), (n, hop, name, float((d / np.maximum(B[:, None], 1e-300)).max()))
            nz = B > 0
            if nz.any():
                worst = max(worst, float((d[nz] / B[nz, None]).max()))
    print("n_fft %d: worst |d| / B_f of the float32 restatement %.3f (|d| / (u A_f) %.2f)" % (n_fft, worst, worst * lm.K(n_fft)))
    assert 0.0 < worst < 1.0


def _frame_samples(y, n, hop, center):
    """The float32 samples under each frame, [F][n]."""
    p = n // 2 if center else 0
    yp = np.pad(np.asarray(y, np.float32), (p, p))
    F = sm.num_frames(len(y), n, hop, center)
    return yp[np.arange(F)[:, None] * hop + np.arange(n)[None, :]]


def test_the_bounds_of_the_other_kinds_hold_for_the_restatement():
    """lin_power at both powers and lin_db through lm.check, fed with float32 values computed from the restatement as the device
    computes them (fmaf(re, re, im * im), sqrt, 10 log10)."""
    n, hop, win, center, T = lm.GRID[2]
    y = lm.signals(T, n)["burst"]
    v32 = (lm.window32(n, win)[None, :] * _frame_samples(y, n, hop, center)).astype(np.float32)
    re, im = lm.fft_f32(v32, n)
    p = (re.astype(np.float64) ** 2 + (im * im).astype(np.float64)).astype(np.float32)
    st = np.stack([re, im], axis=2).reshape(re.shape[0], -1)
    assert lm.check(st, y, "stft", n, hop, win, center) < 1.0
    assert lm.check(p, y, "lin_power", n, hop, win, center, power=2) < 1.0
    assert lm.check(np.sqrt(p), y, "lin_power", n, hop, win, center, power=1) < 1.0
    for top_db in (None, 80.0, 40.0):
        d = (np.float32(10.0) * np.log10(np.maximum(p, np.float32(1e-10)))).astype(np.float32)
        if top_db:
            d = np.maximum(d, d.max() - np.float32(top_db))
        assert lm.check(d, y, "lin_db", n, hop, win, center, power=2, top_db=top_db) <= 1.0
    # a value outside the bound is caught: the check is not vacuous
    bad = p.copy()
    f, k = np.unravel_index(np.argmax(p), p.shape)
    bad[f, k] *= np.float32(1.0 + 1e-4)
    with pytest.raises(AssertionError):
        lm.check(bad, y, "lin_power", n, hop, win, center, power=2)
