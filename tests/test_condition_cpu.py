"""PCM conditioning (mono downmix, peak normalisation, pre-emphasis): what needs no GPU — the float64 model
(tests/condition_model.py) against scipy.signal.lfilter, the new keywords' argument checks before the library loads, and the new
C-ABI struct and symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

from parseoggvorbis_amd import pcm, spectral
from tests import condition_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("a", [0.97, 0.5, 1e-3, 0.999999])
def test_model_preemphasis_equals_lfilter(a):
    sig = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(int(a * 1000))
    a32 = cm.coefficient(a)
    assert a32 == float(np.float32(a)) and 0.0 < a32 < 1.0
    for T in (0, 1, 2, 100003):
        y = rng.standard_normal(T) * 0.3
        want = sig.lfilter([1.0, -a32], [1.0], y) if T else np.zeros(0)
        got = cm.preemphasis(y, a)
        assert got.shape == (T,)
        assert np.abs(got - want).max(initial=0.0) <= 4.0 * np.finfo(np.float64).eps * max(1.0, np.abs(y).max(initial=0.0)), (a, T)
        if T:
            assert got[0] == y[0]


def test_model_peak_and_silence():
    rng = np.random.default_rng(3)
    for C, T in ((1, 1), (2, 1000), (6, 4097)):
        x = rng.standard_normal((C, T)) * 0.2
        y = cm.downmix(x)
        assert np.allclose(y, x.mean(axis=0), rtol=0, atol=1e-15)
        y1 = cm.peak_normalize(y)
        assert np.abs(y1).max() == 1.0  # y / max|y|: the peak sample divides to exactly 1
        assert np.array_equal(cm.peak_normalize(8.0 * y), y1)  # a power of two scales out exactly
        assert np.array_equal(cm.condition(x, True, None), y1)
        assert np.array_equal(cm.condition(x, True, 0.97), cm.preemphasis(y1, 0.97))
        assert np.array_equal(cm.condition(x), y)
    for T in (0, 1, 64):  # silence stays silence, T = 0 is fine
        z = cm.condition(np.zeros((2, T)), True, 0.97)
        assert z.shape == (T,) and not z.any() and cm.peak(np.zeros(T)) == 0.0
    with pytest.raises(ValueError):
        cm.peak_normalize(np.array([0.1, np.inf, 0.2]))
    with pytest.raises(ValueError):
        cm.peak_normalize(np.array([0.1, np.nan]))


def _no_load():
    raise AssertionError("library loaded before the arguments were checked")


BAD = [dict(preemphasis=0), dict(preemphasis=1.0), dict(preemphasis=-0.1), dict(preemphasis=float("nan")), dict(preemphasis=float("inf")),
       dict(preemphasis=True), dict(preemphasis="0.97"), dict(preemphasis=1.0 - 1e-12), dict(preemphasis=1e-60),
       dict(peak_normalize=1), dict(peak_normalize="yes"), dict(peak_normalize=None)]


@pytest.mark.parametrize("kw", [dict(k, mono=True) for k in BAD] +
                         [dict(mono=1), dict(mono="yes"), dict(mono=None), dict(peak_normalize=True, mono=False),
                          dict(preemphasis=0.97, mono=False), dict(peak_normalize=True), dict(preemphasis=0.97)])  # (mono defaults to False)
def test_bad_pcm_arguments_raise_before_the_library_loads(kw, monkeypatch):
    monkeypatch.setattr(pcm, "_load", _no_load)
    with pytest.raises(pcm.PcmError):
        pcm.get_pcm_batch([b"OggS"], **kw)
    with pytest.raises(pcm.PcmError):
        pcm.get_pcm_from_raw_bytes(b"OggS", **kw)


@pytest.mark.parametrize("kw", BAD)
def test_bad_spectral_arguments_raise_before_the_library_loads(kw, monkeypatch):
    monkeypatch.setattr(spectral, "_load", _no_load)
    with pytest.raises(spectral.SpectralError):
        spectral.get_spectral_batch([b"OggS"], **kw)
    with pytest.raises(spectral.SpectralError):
        spectral.get_spectral_from_raw_bytes(b"OggS", **kw)


def test_cond_spec_encoding():
    c = pcm.cond_spec()
    assert (c.options, c.reserved, c.preemphasis) == (0, 0, 0.0)
    c = pcm.cond_spec(True, 0.97)
    assert c.options == 3 and c.preemphasis == float(np.float32(0.97))
    assert pcm.cond_spec(False, np.float32(0.5)).options == 2 and pcm.cond_spec(np.bool_(True)).options == 1


def test_cond_struct_matches_the_header():
    # vsyn_pcm_cond: two uint32, one double
    from parseoggvorbis_amd import binding
    assert ctypes.sizeof(binding.PcmCond) == 16
    assert binding.PcmCond.options.offset == 0 and binding.PcmCond.reserved.offset == 4 and binding.PcmCond.preemphasis.offset == 8
    header = open(os.path.join(ROOT, "include", "vorbis_synth_hip.h")).read()
    m = re.search(r"typedef struct vsyn_pcm_cond \{(.*?)\} vsyn_pcm_cond;", header, flags=re.S)
    fields = re.findall(r"^\s*(uint32_t|double)\s+(\w+);", m.group(1), flags=re.M)
    assert fields == [("uint32_t", "options"), ("uint32_t", "reserved"), ("double", "preemphasis")]
    assert re.search(r"#define VSYN_COND_PEAK 1u", header) and re.search(r"#define VSYN_COND_PREEMPH 2u", header)
    assert (binding.VSYN_COND_PEAK, binding.VSYN_COND_PREEMPH) == (1, 2) == (pcm.COND_PEAK, pcm.COND_PREEMPH)


def test_new_symbols_are_declared_and_exported():
    from parseoggvorbis_amd import binding
    lib = binding.load()
    header = open(os.path.join(ROOT, "include", "vorbis_synth_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for s in ("vsyn_pcm_condition_device", "vsyn_pcm_condition_host", "vsyn_pcm_cond_spectral_host"):
        assert s in binding.declared_symbols() and hasattr(lib, s)
        assert re.search(r"\b%s\s*\(" % s, code), s
    assert "PCM conditioning" in header
    assert lib.vsyn_abi_version() == 5
    host = ctypes.CDLL(pcm.HOST_LIB_PATH)
    assert hasattr(host, "ogg_vorbis_pcm_corpus_cond") and hasattr(host, "ogg_vorbis_spectral_corpus_cond")


def test_new_entries_fail_loudly_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from parseoggvorbis_amd import binding
    lib = binding.load()
    cond = binding.PcmCond(3, 0, 0.97)
    spec = spectral.spectral_spec()
    err = ctypes.c_char_p()
    frames = (ctypes.c_uint64 * 1)()
    rows = (ctypes.c_uint64 * 1)()
    st = binding.Status()
    rcs = [lib.vsyn_pcm_condition_device(None, ctypes.byref(cond), 1, None, 16, 2, None, None, 16, None, None, ctypes.byref(err)),
           lib.vsyn_pcm_condition_host(None, ctypes.byref(cond), 1, None, 0, binding.VSYN_PCM_F32, None, 0, frames, None, ctypes.byref(err)),
           lib.vsyn_pcm_cond_spectral_host(None, ctypes.byref(cond), ctypes.byref(spec), None, 1, None, 0, None, 0, rows, None,
                                           ctypes.byref(st), ctypes.byref(err))]
    assert rcs == [binding.VSYN_ERR_NO_DEVICE] * 3, rcs
    assert b"no CPU path" in err.value
