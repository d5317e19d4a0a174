"""Spectral features (parseoggvorbis_amd/spectral.py): what needs no GPU — argument checks before the library loads, the float64
model (tests/spectral_model.py) against torch.stft / scipy's DCT and the mel scale's defining values, and the new C-ABI symbols."""
import ctypes
import math

import numpy as np
import pytest

from parseoggvorbis_amd import spectral
from tests import spectral_model as sm


@pytest.mark.parametrize("kw", [dict(kind="mfcc_db"), dict(n_fft=8), dict(n_fft=8193), dict(hop_length=0), dict(win_length=0),
                                dict(n_fft=400, win_length=401), dict(n_mels=0), dict(n_mels=257), dict(kind="mfcc", n_mels=10, n_mfcc=11),
                                dict(fmin=-1.0), dict(fmin=4000.0, fmax=3000.0), dict(power=3), dict(power=0.5), dict(norm="l2"),
                                dict(kind="log_mel", log_floor=0.0), dict(kind="mel_db", amin=0.0), dict(kind="mel_db", top_db=-1.0),
                                dict(n_fft=512.0)])
def test_bad_arguments_raise_before_the_library_loads(kw, monkeypatch):
    def no_load():
        raise AssertionError("library loaded before the arguments were checked")
    monkeypatch.setattr(spectral, "_load", no_load)
    with pytest.raises(spectral.SpectralError):
        spectral.get_spectral_batch([b"OggS"], **kw)
    with pytest.raises(spectral.SpectralError):
        spectral.get_spectral_from_raw_bytes(b"OggS", **kw)


def test_bad_kind_names_the_kinds():
    with pytest.raises(spectral.SpectralError) as ei:
        spectral.spectral_spec("spectrogram")
    for k in ("mel_power", "log_mel", "mel_db", "mfcc"):
        assert k in str(ei.value)


def test_spec_encoding():
    s = spectral.spectral_spec()
    assert (s.kind, s.options, s.n_fft, s.hop_length, s.win_length, s.n_mels, s.power) == (2, spectral.OPT_CENTER, 2048, 512, 2048, 128, 2)
    assert (s.fmin, s.fmax, s.log_floor, s.amin, s.top_db) == (0.0, 0.0, 1e-3, 1e-10, 80.0)
    s = spectral.spectral_spec("mfcc", n_fft=400, hop_length=160, n_mels=40, htk=True, norm=None, center=False, power=1, n_mfcc=13,
                               fmin=20.0, fmax=7600.0, top_db=None)
    assert s.options == spectral.OPT_HTK | spectral.OPT_NO_NORM and (s.n_mfcc, s.power, s.top_db) == (13, 1, 0.0)
    assert (s.fmin, s.fmax) == (20.0, 7600.0)
    assert spectral.spec_dim(s) == 13 and spectral.spec_dim(spectral.spectral_spec("mel_db", n_mels=64)) == 64


def test_mel_scale_spot_values():
    assert sm.hz_to_mel(1000.0) == pytest.approx(15.0, abs=1e-12)
    assert sm.hz_to_mel(6400.0) == pytest.approx(42.0, abs=1e-12)
    assert sm.hz_to_mel(500.0) == pytest.approx(7.5, abs=1e-12)
    assert sm.hz_to_mel(1000.0, htk=True) == pytest.approx(2595.0 * math.log10(1.0 + 1000.0 / 700.0), rel=1e-15)
    f = np.array([0.0, 20.0, 440.0, 999.0, 1000.0, 1001.0, 4000.0, 8000.0, 22050.0])
    for htk in (False, True):
        assert np.allclose(sm.mel_to_hz(sm.hz_to_mel(f, htk), htk), f, rtol=1e-12, atol=1e-9)


def test_mel_filters_shape_and_area():
    W = sm.mel_filters(44100, 2048, 128)
    assert W.shape == (128, 1025) and (W >= 0).all()
    for m in range(128):  # every band a single run of positive bins (the device's sparse table relies on it)
        nz = np.flatnonzero(W[m])
        if nz.size:
            assert nz[-1] - nz[0] + 1 == nz.size
    Wn = sm.mel_filters(16000, 400, 40, htk=True, norm=None)
    assert Wn.max() <= 1.0 + 1e-12


@pytest.mark.parametrize("n_fft,hop,win", [(16, 4, None), (400, 160, None), (400, 160, 300), (1102, 441, None), (1102, 441, 882),
                                           (2048, 512, None), (2048, 512, 1500), (401, 100, None), (401, 128, 250)])
def test_model_spectrum_equals_torch_stft(n_fft, hop, win):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(n_fft + hop)
    x = rng.standard_normal((2, 5000))
    for center in (True, False):
        S = sm.spectrum(x, n_fft, hop, win, center=center)
        y = torch.from_numpy(x.mean(axis=0))
        w = torch.from_numpy(sm.window(n_fft, win))
        X = torch.stft(y, n_fft, hop_length=hop, win_length=n_fft, window=w, center=center, pad_mode="constant", onesided=True,
                       return_complex=True)
        want = (X.abs() ** 2).numpy().T
        assert S.shape == want.shape
        assert S.shape[0] == sm.num_frames(5000, n_fft, hop, center)
        assert np.abs(S - want).max() <= 1e-9 * np.abs(want).max()
        if win is None:  # torch's own periodic Hann is the same window
            w2 = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
            X2 = torch.stft(y, n_fft, hop_length=hop, window=w2, center=center, pad_mode="constant", onesided=True, return_complex=True)
            assert np.abs(S - (X2.abs() ** 2).numpy().T).max() <= 1e-9 * np.abs(want).max()


def test_model_frame_counts():
    assert sm.num_frames(0, 2048, 512) == 0
    assert sm.num_frames(384, 2048, 512, center=False) == 0
    assert sm.num_frames(384, 2048, 512, center=True) == 1
    assert sm.num_frames(2048, 2048, 512, center=False) == 1
    assert sm.num_frames(44100, 1102, 441) == 101
    assert sm.spectrum(np.zeros((1, 100)), 2048, 512, center=False).shape == (0, 1025)


def test_model_dct_equals_scipy():
    fft = pytest.importorskip("scipy.fft")
    rng = np.random.default_rng(3)
    for n_mels, n_mfcc in ((128, 20), (40, 13), (80, 80), (7, 1)):
        D = rng.standard_normal((9, n_mels))
        want = fft.dct(D, type=2, norm="ortho", axis=-1)[:, :n_mfcc]
        assert np.abs(D @ sm.dct_ortho(n_mfcc, n_mels).T - want).max() < 1e-12


def test_new_symbols_are_exported():
    from parseoggvorbis_amd import binding
    lib = binding.load()
    for s in ("vsyn_spectral_num_frames", "vsyn_spectral_device", "vsyn_pcm_spectral_host"):
        assert s in binding.declared_symbols() and hasattr(lib, s)
    host = ctypes.CDLL(spectral.HOST_LIB_PATH)
    assert hasattr(host, "ogg_vorbis_spectral_corpus")


def test_spec_struct_matches_the_header():
    # vsyn_spectral_spec: eight uint32, five double
    from parseoggvorbis_amd import binding
    assert ctypes.sizeof(binding.SpectralSpec) == 72
    assert binding.SpectralSpec.fmin.offset == 32 and binding.SpectralSpec.top_db.offset == 64


def test_library_frame_count_equals_the_model():
    from parseoggvorbis_amd import binding
    lib = binding.load()
    for kw in (dict(), dict(n_fft=1102, hop_length=441), dict(n_fft=401, hop_length=100, center=False), dict(n_fft=16, hop_length=3)):
        s = spectral.spectral_spec(**kw)
        for T in (0, 1, 15, 16, 383, 384, 1101, 1102, 2047, 2048, 2049, 44100, 1 << 24):
            want = sm.num_frames(T, s.n_fft, s.hop_length, bool(s.options & spectral.OPT_CENTER))
            assert lib.vsyn_spectral_num_frames(ctypes.byref(s), T) == want, (kw, T)
    bad = spectral.spectral_spec()
    bad.n_fft = 9000
    assert lib.vsyn_spectral_num_frames(ctypes.byref(bad), 44100) == 0
