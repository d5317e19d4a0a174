"""Chroma and tonnetz (include/vorbis_synth_hip.h, "chroma"): what needs no GPU — properties of the float64 model
(tests/chroma_model.py), the library's host-built filterbank against it (vsyn_chroma_filterbank needs no device), the kinds' encoding
and dim on both sides of the C ABI, and every argument check before the library loads."""
import ctypes
import math

import numpy as np
import pytest

from parseoggvorbis_amd import spectral
from tests import chroma_model as cm
from tests import spectral_lin_model as lm


# ---- the model ----

@pytest.mark.parametrize("n_chroma", [12, 13, 36])
def test_without_octave_weighting_every_column_has_unit_l2_norm(n_chroma):
    for sr, n_fft in ((22050, 2048), (8000, 48)):
        W = cm.filterbank(sr, n_fft, n_chroma, tuning=0.37, octwidth=None)
        assert W.shape == (n_chroma, n_fft // 2 + 1)
        assert np.allclose(np.sqrt((W * W).sum(axis=0)), 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("n_chroma", [12, 13, 36])
def test_base_c_is_the_stated_rotation(n_chroma):
    a = cm.filterbank(22050, 400, n_chroma, base_c=False)
    c = cm.filterbank(22050, 400, n_chroma, base_c=True)
    rot = 3 * (n_chroma // 12)
    for r in range(n_chroma):
        assert np.array_equal(c[r], a[(r + rot) % n_chroma])


def test_windowed_sines_peak_in_their_pitch_class():
    sr, n = 22050, 2048
    t = np.arange(n) / sr
    for hz, row in ((440.0, 9), (261.63, 0), (329.63, 4)):
        want, _ = cm.rows(np.sin(2 * np.pi * hz * t), "chroma", sr, n, n, center=False)
        assert want.shape == (1, 12) and int(np.argmax(want[0])) == row and want[0].max() == pytest.approx(1.0)


def test_n_chroma_13_uses_h_6():
    """rint(6.5) = 6 (ties to even), not 7: D lies in [-6, 7), and the two choices differ."""
    n_chroma, sr, n_fft = 13, 22050, 400
    W = cm.filterbank(sr, n_fft, n_chroma, octwidth=None, base_c=False)
    q = n_chroma * np.log2((np.arange(1, n_fft) * sr / n_fft) / (440.0 / 16.0))
    bw = np.concatenate([np.maximum(q[1:] - q[:-1], 1.0), [1.0]])
    for h, same in ((6.0, True), (7.0, False)):
        D = np.remainder(q[None, :] - np.arange(n_chroma)[:, None] + h + 10 * n_chroma, n_chroma) - h
        G = np.exp(-0.5 * (2 * D / bw[None, :]) ** 2)
        G = (G / np.sqrt((G * G).sum(axis=0))[None, :])[:, :n_fft // 2]
        assert np.allclose(G, W[:, 1:], rtol=1e-12, atol=0) == same, h


@pytest.mark.parametrize("n_chroma", [12, 36])
def test_tonnetz_of_a_one_hot_row_is_the_column_of_phi(n_chroma):
    P = cm.phi(n_chroma)
    assert P.shape == (6, n_chroma)
    for c in range(n_chroma):
        R = np.zeros((1, n_chroma))
        R[0, c] = 3.5
        for norm in (0, 1, 2, 3):
            row, _ = cm.normalize(R, np.zeros_like(R), norm)
            u, _ = cm.normalize(row, np.zeros_like(R), 1)
            assert np.allclose(u @ P.T, P[:, c][None, :], rtol=0, atol=1e-15)
    assert np.allclose(cm.phi(12)[:, 0], [0.0, 1.0, 0.0, 1.0, 0.0, 0.5], atol=1e-15)  # r_i cos(-pi o_i)


def test_the_non_finite_rule_and_silence_in_the_model():
    y = np.zeros(64 * 6)
    y[64:128] = np.random.default_rng(0).standard_normal(64)
    y[200] = np.nan
    for kind in ("chroma", "tonnetz"):
        for norm in (None, 1, 2, np.inf):
            want, tol = cm.rows(y, kind, 8000, 64, 64, center=False, chroma_norm=norm)
            assert np.isnan(want[3]).all() and np.isfinite(np.delete(want, 3, axis=0)).all()
            assert (want[[0, 2, 4, 5]] == 0).all() and (tol[[0, 2, 4, 5]] == 0).all() and np.abs(want[1]).max() > 0


# ---- the library's table against the model ----

@pytest.fixture(scope="module")
def lib():
    from parseoggvorbis_amd import binding
    return binding.load()


def _table(lib, sr, spec, chroma):
    out = np.full((12 if chroma is None else chroma.n_chroma, spec.n_fft // 2 + 1), np.nan, np.float32)
    rc = lib.vsyn_chroma_filterbank(sr, ctypes.byref(spec), None if chroma is None else ctypes.byref(chroma), out.ctypes.data)
    return rc, out


@pytest.mark.parametrize("n_fft", [16, 48, 400, 2048, 8192])
@pytest.mark.parametrize("sr", [8000, 22050, 44100])
def test_the_filterbank_table_against_the_model(lib, sr, n_fft):
    """|table - model| <= 2^-23 |model| + FLT_MIN: one float32 rounding of a double whose libm may differ from numpy's by an ulp, and
    the flush of what is below FLT_MIN. No denormal is stored."""
    spec = spectral.spectral_spec("chroma", n_fft=n_fft, hop_length=n_fft // 4)
    for n_chroma in (12, 13, 36):
        for tuning in (0.0, 0.37, -0.37):
            for octwidth in (2.0, None):
                for base_c in (True, False):
                    ch = spectral.chroma_spec(n_chroma, tuning, np.inf, 5.0, octwidth, base_c)
                    rc, got = _table(lib, sr, spec, ch)
                    assert rc == 0
                    want = cm.filterbank(sr, n_fft, n_chroma, tuning, 5.0, octwidth, base_c)
                    assert (np.abs(got.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want) + cm.FLT_MIN).all(), (n_chroma, tuning, octwidth, base_c)
                    assert ((got == 0) | (np.abs(got) >= np.float32(cm.FLT_MIN))).all()


def test_the_default_table_and_the_refusals_of_the_table_entry(lib):
    spec = spectral.spectral_spec("tonnetz", n_fft=400, hop_length=100)
    rc, got = _table(lib, 22050, spectral.spectral_spec("chroma", n_fft=400, hop_length=100), None)
    assert rc == 0 and np.array_equal(got, _table(lib, 22050, spec, spectral.chroma_spec())[1][:12])
    assert np.abs(got.astype(np.float64) - cm.filterbank(22050, 400)).max() < 1e-6 and got.max() > 0.1
    out = np.zeros((12, 201), np.float32)
    assert lib.vsyn_chroma_filterbank(0, ctypes.byref(spec), None, out.ctypes.data) != 0
    assert lib.vsyn_chroma_filterbank(22050, ctypes.byref(spec), None, None) != 0
    assert lib.vsyn_chroma_filterbank(22050, ctypes.byref(spectral.spectral_spec("lin_power", n_fft=400)), None, out.ctypes.data) != 0
    bad = spectral.chroma_spec()
    bad.norm = 4
    assert lib.vsyn_chroma_filterbank(22050, ctypes.byref(spec), ctypes.byref(bad), out.ctypes.data) != 0
    assert (out == 0).all()


# ---- kinds, dims and checks on both sides of the C ABI ----

def test_the_kinds_encode_8_and_9_and_their_dims(lib):
    from parseoggvorbis_amd import binding
    assert (spectral.CHROMA_KINDS["chroma"], spectral.CHROMA_KINDS["tonnetz"]) == (8, 9) == (binding.VSYN_SPEC_CHROMA, binding.VSYN_SPEC_TONNETZ)
    assert spectral.ALL_KINDS == dict(spectral.KINDS, chroma=8, tonnetz=9) and "chroma" not in spectral.KINDS
    assert ctypes.sizeof(binding.SpectralChroma) == 40 and lib.vsyn_abi_version() == 5
    for name in ("vsyn_spectral_chroma_dim", "vsyn_chroma_filterbank", "vsyn_spectral_chroma_tile", "vsyn_spectral_chroma_device",
                 "vsyn_pcm_chain_chroma_host"):
        assert name in binding.declared_symbols()
    d = spectral.chroma_spec()
    assert (d.n_chroma, d.norm, d.options, d.tuning, d.ctroct, d.octwidth) == (12, 3, 1, 0.0, 5.0, 2.0)
    for n_fft in (16, 1102, 8192):
        c = spectral.spectral_spec("chroma", n_fft=n_fft, hop_length=4)
        t = spectral.spectral_spec("tonnetz", n_fft=n_fft, hop_length=4)
        assert (c.kind, t.kind) == (8, 9)
        # vsyn_spectral_dim takes no chroma parameters and keeps its answer for these codes; the chroma form sizes their rows
        assert lib.vsyn_spectral_dim(ctypes.byref(c)) == spectral.spec_dim(c) == 0
        assert lib.vsyn_spectral_dim(ctypes.byref(t)) == spectral.spec_dim(t) == 0
        assert lib.vsyn_spectral_chroma_dim(ctypes.byref(t), None) == spectral.spec_dim(t, spectral.chroma_spec()) == 6
        assert binding._spec_dim(c) == 12 and binding._spec_dim(t) == 6  # (what the entries without the chroma argument write)
        for n_chroma in (1, 13, 256):
            ch = spectral.chroma_spec(n_chroma)
            assert lib.vsyn_spectral_chroma_dim(ctypes.byref(c), ctypes.byref(ch)) == spectral.spec_dim(c, ch) == n_chroma
            assert lib.vsyn_spectral_chroma_dim(ctypes.byref(t), ctypes.byref(ch)) == spectral.spec_dim(t, ch) == 6
        assert lib.vsyn_spectral_chroma_dim(ctypes.byref(c), None) == spectral.spec_dim(c, spectral.chroma_spec()) == 12
        assert lib.vsyn_spectral_chroma_tile(ctypes.byref(c)) >= 1
        assert lib.vsyn_spectral_lin_tile(ctypes.byref(c)) == 0
    m = spectral.spectral_spec("mel_power", n_mels=40)
    assert lib.vsyn_spectral_chroma_dim(ctypes.byref(m), None) == 40 and lib.vsyn_spectral_chroma_tile(ctypes.byref(m)) == 0
    # the post stage takes these rows; the mel fields, amin, top_db and log_floor are neither read nor checked
    on, _, _ = spectral.post_spec(12, delta=2)
    c = spectral.spectral_spec("chroma", n_fft=64, hop_length=8)
    assert lib.vsyn_spectral_post_dim(ctypes.byref(c), ctypes.byref(on)) == 36
    c.n_mels, c.n_mfcc, c.fmin, c.fmax, c.log_floor, c.amin, c.top_db = 0, 999, -5.0, 1.0, -1.0, -1.0, -1.0
    assert lib.vsyn_spectral_chroma_dim(ctypes.byref(c), None) == 12
    c.power = 3
    assert lib.vsyn_spectral_chroma_dim(ctypes.byref(c), None) == 0


def test_the_library_checks_the_chroma_struct(lib):
    c = spectral.spectral_spec("chroma", n_fft=64, hop_length=8)
    for field, value in (("n_chroma", 0), ("n_chroma", 257), ("norm", 4), ("options", 4), ("tuning", math.nan), ("tuning", math.inf),
                         ("ctroct", math.nan), ("octwidth", 0.0), ("octwidth", -1.0), ("octwidth", math.nan), ("octwidth", math.inf)):
        ch = spectral.chroma_spec()
        setattr(ch, field, value)
        assert lib.vsyn_spectral_chroma_dim(ctypes.byref(c), ctypes.byref(ch)) == 0, (field, value)
    ch = spectral.chroma_spec(octwidth=None)
    ch.octwidth = math.nan  # not read with VSYN_CHROMA_NO_OCT
    assert lib.vsyn_spectral_chroma_dim(ctypes.byref(c), ctypes.byref(ch)) == 12
    for field, value in (("n_fft", 15), ("n_fft", 8193), ("hop_length", 0), ("win_length", 0), ("win_length", 65), ("options", 8), ("power", 0)):
        s = spectral.spectral_spec("tonnetz", n_fft=64, hop_length=8)
        setattr(s, field, value)
        assert lib.vsyn_spectral_chroma_dim(ctypes.byref(s), None) == 0, (field, value)


BAD_ARGS = [dict(n_chroma=0), dict(n_chroma=257), dict(n_chroma=12.0), dict(n_chroma=True), dict(tuning=None), dict(tuning=math.nan),
            dict(tuning=math.inf), dict(tuning="a"), dict(chroma_norm=0), dict(chroma_norm=3), dict(chroma_norm="max"), dict(chroma_norm=True),
            dict(chroma_norm=-math.inf), dict(ctroct=None), dict(ctroct=math.nan), dict(octwidth=0.0), dict(octwidth=-2.0), dict(octwidth=math.inf),
            dict(octwidth=math.nan), dict(base_c=1), dict(base_c=None)]


@pytest.mark.parametrize("kw", BAD_ARGS, ids=lambda kw: "%s=%r" % next(iter(kw.items())))
@pytest.mark.parametrize("kind", ["chroma", "tonnetz", "log_mel"])
def test_every_chroma_argument_is_checked_before_the_library_loads(kind, kw, monkeypatch):
    def no_load():
        raise AssertionError("library loaded before the arguments were checked")
    monkeypatch.setattr(spectral, "_load", no_load)
    with pytest.raises(spectral.SpectralError) as ei:
        spectral.get_spectral_batch([b"OggS"], kind=kind, n_fft=64, hop_length=16, **kw)
    assert next(iter(kw)) in str(ei.value)
    with pytest.raises(spectral.SpectralError):
        spectral.get_spectral_from_raw_bytes(b"OggS", kind=kind, **kw)


@pytest.mark.parametrize("kind", ["chroma", "tonnetz"])
def test_the_spectral_checks_and_pcen_raise_before_the_library_loads(kind, monkeypatch):
    def no_load():
        raise AssertionError("library loaded before the arguments were checked")
    monkeypatch.setattr(spectral, "_load", no_load)
    for kw in (dict(pcen=True), dict(n_fft=8), dict(n_fft=9000), dict(hop_length=0), dict(win_length=0), dict(win_length=4096), dict(power=3),
               dict(delta=3), dict(normalize="max")):
        with pytest.raises(spectral.SpectralError):
            spectral.get_spectral_batch([b"OggS"], kind=kind, **kw)
    with pytest.raises(spectral.SpectralError) as ei:
        spectral.get_spectral_batch([b"OggS"], kind=kind, pcen=True)
    assert "pcen" in str(ei.value) and kind in str(ei.value)


def test_accepted_forms_of_the_chroma_arguments():
    assert [spectral.chroma_spec(chroma_norm=n).norm for n in (None, 1, 2, np.inf, math.inf, np.float64(2.0), np.int64(1))] == [0, 1, 2, 3, 3, 2, 1]
    ch = spectral.chroma_spec(36, -0.37, 2, 4.0, None, False)
    assert (ch.n_chroma, ch.norm, ch.options, ch.tuning, ch.ctroct) == (36, 2, 2, -0.37, 4.0)
    assert spectral.chroma_spec(base_c=np.bool_(True)).options == 1
