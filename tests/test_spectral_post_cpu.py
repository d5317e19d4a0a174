"""Spectral post-processing (delta columns, mean / variance normalisation): what needs no GPU — the float64 model
(tests/spectral_post_model.py) against scipy.signal.savgol_filter, the new keywords' argument checks before the library loads, and the
new C-ABI symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

from parseoggvorbis_amd import spectral
from tests import spectral_post_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("width", [3, 5, 9, 65])
@pytest.mark.parametrize("order", [1, 2])
def test_model_deltas_equal_savgol(width, order):
    sig = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(width * 10 + order)
    for F in (width, width + 1, width + 2, 2 * width + 1, 37 + width, 300):
        x = rng.standard_normal((F, 5)) * 3.0 + 1.0
        want = sig.savgol_filter(x, width, deriv=order, polyorder=order, axis=0, mode="interp")
        got = pm.delta(x, width, order)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (width, order, F)


def test_model_shapes_and_short_input():
    x = np.arange(40.0).reshape(10, 4)
    assert pm.with_deltas(x, 0).shape == (10, 4) and pm.with_deltas(x, 2).shape == (10, 12)
    assert pm.with_deltas(x[:0], 2).shape == (0, 12)
    with pytest.raises(ValueError):
        pm.with_deltas(x[:8], 1, 9)
    # a ramp: the first derivative is its slope, the second is zero, at the edges too
    y = pm.with_deltas(x, 2, 9)
    assert np.allclose(y[:, 4:8], 4.0, atol=1e-12) and np.allclose(y[:, 8:], 0.0, atol=1e-12)


def test_model_normalisation():
    rng = np.random.default_rng(1)
    y = rng.standard_normal((50, 6)) * np.array([1, 2, 3, 1e-2, 5, 0.0]) + np.array([0, 1, -1, 1e3, 7, 4.0])
    z = pm.normalize(y, "mean_var")
    assert np.abs(z.mean(axis=0)).max() < 1e-9 and np.allclose(z[:, :5].std(axis=0), 1.0) and (z[:, 5] == 0).all()
    assert np.allclose(pm.normalize(y, "mean"), y - y.mean(axis=0))
    mean, std = np.arange(6.0), np.array([1, 2, 4, 1e-9, 1, 1.0])
    z = pm.normalize(y, given=(mean, std), std_floor=0.5)
    assert np.allclose(z, (y - mean) / np.maximum(std, 0.5))
    assert np.array_equal(pm.normalize(y, given=(mean, None)), y - mean)
    assert np.array_equal(pm.post(y, 0, 9, None), y)


@pytest.mark.parametrize("kw", [dict(delta=1, delta_width=8), dict(delta=1, delta_width=1), dict(delta_width=4), dict(delta=3),
                                dict(delta=-1), dict(delta=1.0), dict(delta=1, delta_width=67), dict(std_floor=0.0),
                                dict(std_floor=-1e-5), dict(std_floor=float("inf")), dict(std_floor=None), dict(normalize="var"),
                                dict(normalize=True), dict(normalize=(np.zeros(128),)),
                                dict(normalize=(np.zeros(127), np.ones(127))), dict(normalize=(np.zeros(128), np.ones(129))),
                                dict(delta=1, normalize=(np.zeros(128), np.ones(128))),
                                dict(delta=2, normalize=(np.zeros(384), np.ones(128))),
                                dict(normalize=(np.full(128, np.nan), None)), dict(normalize=(np.zeros(128), np.full(128, np.inf))),
                                dict(normalize=(None, np.ones(128))), dict(kind="mfcc", n_mfcc=13, delta=2, normalize=(np.zeros(13), None))])
def test_bad_post_arguments_raise_before_the_library_loads(kw, monkeypatch):
    def no_load():
        raise AssertionError("library loaded before the arguments were checked")
    monkeypatch.setattr(spectral, "_load", no_load)
    with pytest.raises(spectral.SpectralError):
        spectral.get_spectral_batch([b"OggS"], **kw)
    with pytest.raises(spectral.SpectralError):
        spectral.get_spectral_from_raw_bytes(b"OggS", **kw)


def test_post_spec_encoding():
    assert spectral.post_spec(80) == (None, 80, ())
    p, dout, keep = spectral.post_spec(80, delta=2, normalize="mean_var", std_floor=1e-3)
    assert (p.order, p.width, p.norm, p.stats, p.std_floor, dout, keep) == (2, 9, 2, 0, 1e-3, 240, ())
    assert p.mean is None and p.std is None
    p, dout, keep = spectral.post_spec(13, delta=1, delta_width=5, normalize=(list(range(26)), None))
    assert (p.order, p.width, p.norm, p.stats, dout) == (1, 5, 1, 1, 26) and p.std is None
    assert p.mean == keep[0].ctypes.data and keep[0].dtype == np.float32
    p, dout, keep = spectral.post_spec(4, normalize=(np.zeros(4), np.ones(4)))
    assert (p.order, p.norm, p.stats, dout) == (0, 2, 1, 4) and p.std == keep[1].ctypes.data


def test_post_struct_matches_the_header():
    # vsyn_spectral_post: four uint32, one double, two pointers
    from parseoggvorbis_amd import binding
    assert ctypes.sizeof(binding.SpectralPost) == 40
    assert binding.SpectralPost.std_floor.offset == 16 and binding.SpectralPost.mean.offset == 24 and binding.SpectralPost.std.offset == 32


def test_new_symbols_are_declared_and_exported():
    from parseoggvorbis_amd import binding
    lib = binding.load()
    header = open(os.path.join(ROOT, "include", "vorbis_synth_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for s in ("vsyn_spectral_post_dim", "vsyn_spectral_post_device", "vsyn_pcm_spectral_post_host"):
        assert s in binding.declared_symbols() and hasattr(lib, s)
        assert re.search(r"\b%s\s*\(" % s, code), s
    assert "spectral post-processing" in header
    assert lib.vsyn_abi_version() == 5
    host = ctypes.CDLL(spectral.HOST_LIB_PATH)
    assert hasattr(host, "ogg_vorbis_spectral_corpus_post")


def test_library_post_dim_and_checks():
    from parseoggvorbis_amd import binding
    lib = binding.load()
    mfcc, mel = spectral.spectral_spec("mfcc", n_mfcc=13), spectral.spectral_spec("log_mel", n_mels=80)
    P = binding.SpectralPost
    assert lib.vsyn_spectral_post_dim(ctypes.byref(mfcc), ctypes.byref(P(2, 9, 2, 0, 1e-5, None, None))) == 39
    assert lib.vsyn_spectral_post_dim(ctypes.byref(mel), ctypes.byref(P(0, 9, 1, 0, 1e-5, None, None))) == 80
    assert lib.vsyn_spectral_post_dim(ctypes.byref(mel), ctypes.byref(P(1, 65, 0, 0, 1e-5, None, None))) == 160
    for bad in (P(3, 9, 0, 0, 1e-5, None, None), P(1, 8, 0, 0, 1e-5, None, None), P(1, 1, 0, 0, 1e-5, None, None),
                P(1, 67, 0, 0, 1e-5, None, None), P(0, 9, 3, 0, 1e-5, None, None), P(0, 9, 1, 2, 1e-5, None, None),
                P(0, 9, 2, 0, 0.0, None, None), P(0, 9, 2, 0, float("nan"), None, None), P(0, 9, 2, 1, 1e-5, None, None)):
        assert lib.vsyn_spectral_post_dim(ctypes.byref(mel), ctypes.byref(bad)) == 0
    broken = spectral.spectral_spec()
    broken.n_fft = 9000
    assert lib.vsyn_spectral_post_dim(ctypes.byref(broken), ctypes.byref(P(1, 9, 0, 0, 1e-5, None, None))) == 0
