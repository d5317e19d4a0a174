"""PCEN (include/vorbis_synth_hip.h, "PCEN"): what needs no GPU — the float64 model (tests/pcen_model.py) against a restatement in
librosa's own words (scipy.signal.lfilter with lfilter_zi, and librosa's three output expressions), the coefficient, a NumPy
restatement of the device's blocked order inside the gate of the GPU test (so that the gate is neither vacuous nor too tight before
any GPU run), the argument checks before the library loads, and the encoding on both sides of the C ABI."""
import ctypes
import os

import numpy as np
import pytest
import scipy.signal

from parseoggvorbis_amd import spectral
from tests import pcen_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["vsyn_spectral_pcen_b", "vsyn_spectral_pcen_device", "vsyn_pcm_trim_spectral_pcen_host", "vsyn_pcm_split_spectral_pcen_host"]


def _librosa_words(X, sr, hop_length, gain, bias, power, time_constant, eps, b, scale):
    """librosa.pcen (0.10, max_size=1) on S = X.T * scale, statement by statement, transposed back: (F, D) float64."""
    S = (np.asarray(X, np.float32) * np.float32(scale)).astype(np.float32).astype(np.float64).T
    if b is None:
        t_frames = time_constant * sr / float(hop_length)
        b = (np.sqrt(1 + 4 * t_frames ** 2) - 1) / (2 * t_frames ** 2)
    # "if zi is None: zi = np.empty(shape); zi[:] = scipy.signal.lfilter_zi([b], [1, b - 1])[:]": 1 - b, not scaled by S[..., 0]
    zi = np.repeat(scipy.signal.lfilter_zi([b], [1, b - 1])[None, :], S.shape[0], axis=0)
    S_smooth, _ = scipy.signal.lfilter([b], [1, b - 1], S, zi=zi, axis=-1)
    with np.errstate(all="ignore"):
        smooth = np.exp(-gain * (np.log(eps) + np.log1p(S_smooth / eps)))
        if power == 0:
            S_out = np.log1p(S * smooth)
        elif bias == 0:
            S_out = np.exp(power * (np.log(S) + np.log(smooth)))
        else:
            S_out = (bias ** power) * np.expm1(power * np.log1p(S * smooth / bias))
    return S_out.T


@pytest.mark.parametrize("i", range(len(pm.PARAMS)))
@pytest.mark.parametrize("scale", [1.0, 2.0 ** 31])
def test_model_equals_lfilter_and_librosas_expressions(i, scale):
    kw = dict(pm.DEFAULTS, sr=16000, hop_length=160, scale=scale, **pm.PARAMS[i])
    for F in (1, 2, 65, 300):
        X = pm.rows(F, 5, seed=F, scale=scale)
        want = _librosa_words(X, **kw)
        got = pm.pcen64(X, **kw)
        assert got.shape == want.shape == (F, 5)
        assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), (F, float(np.abs(got / want - 1)[want != 0].max()))


def test_the_coefficient_is_the_closed_form_and_b_1_is_the_input():
    for tc, sr, hop in ((0.4, 22050, 512), (0.4, 16000, 160), (0.06, 44100, 256), (1.5, 8000, 80)):
        t = tc * sr / hop
        b = pm.coefficient(tc, sr, hop)
        assert 0.0 < b < 1.0
        # b solves b^2 t^2 + b - 1 = 0 (librosa's derivation: the first-order filter whose time constant is t frames)
        assert abs(b * b * t * t + b - 1.0) <= 1e-12
    X = pm.rows(100, 4, seed=1)
    assert np.array_equal(pm.smooth(pm.scaled(X, 1.0), 1.0), X.astype(np.float64))


def test_a_constant_column_converges_and_no_rows_give_no_rows():
    S = np.full((4000, 3), 7.25, np.float32)
    M = pm.smooth(S, 0.02)
    assert abs(M[0, 0] - (0.02 * 7.25 + 0.98)) < 1e-15 and np.all(np.diff(M[:, 0]) >= 0) and M[100, 0] < 7.25
    assert np.abs(M[-1] - 7.25).max() < 1e-12 * 7.25 * 1e3  # (1 - b)^4000 of the initial gap
    assert pm.pcen(np.zeros((0, 6), np.float32)).shape == (0, 6) and pm.pcen(np.zeros((0, 6), np.float32)).dtype == np.float32
    assert pm.blocked(np.zeros((0, 6), np.float32)).shape == (0, 6)


@pytest.mark.parametrize("i", range(len(pm.PARAMS)))
def test_the_blocked_order_of_the_device_is_within_the_gate(i):
    """part, carry with q^64, apply, one float32 rounding: tests/pcen_model.py blocked() against the model under the GPU test's gate.
    Over all parameter sets the worst |d| / (u |Y|) is the one rounding: between 0.9 and 1."""
    worst = 0.0
    for scale in (1.0, 2.0 ** 31):
        kw = dict(pm.DEFAULTS, sr=16000, hop_length=160, scale=scale, **pm.PARAMS[i])
        for F in (1, 2, 63, 64, 65, 129, 1000):
            X = pm.rows(F, 6, seed=1000 + F, scale=scale)
            worst = max(worst, pm.gate(pm.blocked(X, **kw), X, **kw))
    print("parameter set %d: worst |d| / (u |Y|) of the blocked restatement %.3f" % (i, worst))
    assert 0.5 < worst <= 1.0 + 1e-6


def test_the_gate_is_not_vacuous():
    kw = dict(pm.DEFAULTS, sr=16000, hop_length=160)
    X = pm.rows(130, 4, seed=3)
    Y = pm.pcen(X, **kw)
    pm.gate(Y, X, **kw)
    bad = Y.copy()
    bad[100, 2] = np.nextafter(np.nextafter(np.nextafter(bad[100, 2], np.float32(np.inf)), np.float32(np.inf)), np.float32(np.inf))
    with pytest.raises(AssertionError):
        pm.gate(bad, X, **kw)
    # the smoother started from 0 instead of 1, or a carry dropped at a block boundary, is caught as well
    S = pm.scaled(X, 1.0)
    M = pm.smooth(S, pm.coefficient(0.4, 16000, 160))
    M0 = M - (1.0 - pm.coefficient(0.4, 16000, 160)) ** np.arange(1, 131)[:, None]
    with pytest.raises(AssertionError):
        pm.gate(pm.compress(S, M0, 0.98, 2.0, 0.5, 1e-6).astype(np.float32), X, **kw)


def test_a_nan_poisons_the_rest_of_its_column_only():
    X = pm.rows(200, 3, seed=9)
    X[70, 1] = np.nan
    Y, B = pm.pcen(X), pm.blocked(X)
    assert np.isnan(Y[70:, 1]).all() and np.isfinite(Y[:70, 1]).all() and np.isfinite(Y[:, [0, 2]]).all()
    assert np.array_equal(np.isnan(B), np.isnan(Y))


BAD = [dict(pcen_gain=-0.1), dict(pcen_gain=float("inf")), dict(pcen_gain=float("nan")), dict(pcen_bias=-1.0), dict(pcen_bias=float("nan")),
       dict(pcen_power=-0.5), dict(pcen_power=float("inf")), dict(pcen_eps=0.0), dict(pcen_eps=-1e-6), dict(pcen_eps=float("inf")),
       dict(pcen_time_constant=0.0), dict(pcen_time_constant=-0.4), dict(pcen_time_constant=float("nan")), dict(pcen_scale=0.0),
       dict(pcen_scale=-1.0), dict(pcen_scale=float("inf")), dict(pcen_b=0.0), dict(pcen_b=-0.1), dict(pcen_b=1.0001),
       dict(pcen_b=float("nan")), dict(pcen_gain=True), dict(pcen_b=True), dict(pcen_scale=False), dict(pcen_eps="1e-6"), dict(pcen=1),
       dict(kind="log_mel"), dict(kind="mel_db"), dict(kind="mfcc"), dict(kind="lin_db"), dict(kind="stft")]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join("%s=%r" % it for it in kw.items()))
def test_bad_keywords_raise_before_the_library_loads(kw, monkeypatch):
    def no_load():
        raise AssertionError("library loaded before the arguments were checked")
    monkeypatch.setattr(spectral, "_load", no_load)
    args = dict(dict(kind="mel_power", pcen=True, n_fft=64, hop_length=16, n_mels=8, n_mfcc=4), **kw)
    with pytest.raises(spectral.SpectralError):
        spectral.get_spectral_batch([b"OggS"], **args)
    with pytest.raises(spectral.SpectralError):
        spectral.get_spectral_from_raw_bytes(b"OggS", **args)


def test_the_kind_refusal_names_the_kind_and_good_keywords_reach_the_library(monkeypatch):
    class Reached(Exception):
        pass

    def no_load():
        raise Reached()
    monkeypatch.setattr(spectral, "_load", no_load)
    with pytest.raises(spectral.SpectralError) as ei:
        spectral.get_spectral_batch([b"OggS"], kind="log_mel", pcen=True)
    assert "log_mel" in str(ei.value) and "mel_power" in str(ei.value)
    for kind in ("mel_power", "lin_power"):
        with pytest.raises(Reached):
            spectral.get_spectral_batch([b"OggS"], kind=kind, pcen=True, pcen_b=1.0, pcen_bias=0, pcen_power=0, pcen_gain=0, pcen_scale=2 ** 31)
    with pytest.raises(spectral.SpectralError):  # the linear kinds still refuse the post stage, with or without PCEN
        spectral.get_spectral_batch([b"OggS"], kind="lin_power", pcen=True, delta=1)
    with pytest.raises(Reached):
        spectral.get_spectral_batch([b"OggS"], kind="mel_power", pcen=True, delta=1, normalize="mean")


def test_pcen_spec_encoding_and_layout():
    from parseoggvorbis_amd import binding
    assert ctypes.sizeof(binding.SpectralPcen) == 56
    names = ["gain", "bias", "power", "time_constant", "eps", "b", "scale"]
    assert [f[0] for f in binding.SpectralPcen._fields_] == names
    assert [getattr(binding.SpectralPcen, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 48]
    p = spectral.pcen_spec()
    assert [getattr(p, n) for n in names] == [0.98, 2.0, 0.5, 0.4, 1e-6, 0.0, 1.0]
    p = spectral.pcen_spec(gain=0, bias=0, power=0, time_constant=2, eps=1e-12, b=1, scale=2 ** 31)
    assert [getattr(p, n) for n in names] == [0.0, 0.0, 0.0, 2.0, 1e-12, 1.0, 2.0 ** 31]
    assert spectral.pcen_spec(b=np.float32(0.5)).b == 0.5


def test_symbols_are_declared_exported_and_in_the_header():
    from parseoggvorbis_amd import binding
    lib = binding.load()
    header = open(os.path.join(ROOT, "include", "vorbis_synth_hip.h")).read()
    assert "PCEN" in header and "typedef struct vsyn_spectral_pcen" in header
    for s in SYMBOLS:
        assert s in binding.declared_symbols() and hasattr(lib, s)
        assert s + "(" in header, s
    assert lib.vsyn_abi_version() == 5
    host = ctypes.CDLL(spectral.HOST_LIB_PATH)
    assert hasattr(host, "ogg_vorbis_spectral_corpus_pcen")


def test_library_coefficient_against_the_model_and_zero_for_an_invalid_spec():
    from parseoggvorbis_amd import binding
    lib = binding.load()
    for tc, sr, hop in ((0.4, 22050, 512), (0.4, 16000, 160), (0.06, 44100, 256), (1.5, 8000, 80), (0.4, 44100, 1)):
        got = lib.vsyn_spectral_pcen_b(ctypes.byref(spectral.pcen_spec(time_constant=tc)), sr, hop)
        want = pm.coefficient(tc, sr, hop)
        assert abs(got - want) <= 1e-14 * want, (tc, sr, hop, got, want)
    assert lib.vsyn_spectral_pcen_b(ctypes.byref(spectral.pcen_spec(b=0.25)), 0, 0) == 0.25
    assert lib.vsyn_spectral_pcen_b(ctypes.byref(spectral.pcen_spec()), 0, 160) == 0.0
    assert lib.vsyn_spectral_pcen_b(ctypes.byref(spectral.pcen_spec()), 16000, 0) == 0.0
    assert lib.vsyn_spectral_pcen_b(None, 16000, 160) == 0.0
    for field, values in (("gain", (-1.0, np.inf, np.nan)), ("bias", (-1.0, np.inf, np.nan)), ("power", (-1.0, np.inf, np.nan)),
                          ("eps", (0.0, -1.0, np.inf, np.nan)), ("time_constant", (0.0, -1.0, np.inf, np.nan)),
                          ("scale", (0.0, -1.0, np.inf, np.nan)), ("b", (-0.5, 1.5, np.inf, np.nan))):
        for v in values:
            p = spectral.pcen_spec()
            setattr(p, field, v)
            assert lib.vsyn_spectral_pcen_b(ctypes.byref(p), 16000, 160) == 0.0, (field, v)
