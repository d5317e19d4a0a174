"""The HPSS stage without a GPU: the float64 model (tests/hpss_model.py) against independent restatements, the Python layer's
argument checks, and the C ABI's new names."""
import ctypes
import os

import numpy as np
import pytest

from parseoggvorbis_amd import spectral

from . import hpss_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["vsyn_spectral_hpss_device", "vsyn_pcm_chain_hpss_host"]
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 3), (3, 2), (7, 9), (30, 17), (40, 33), (70, 5)]


def pad_sort_median(X, k, axis):
    """The definition in numpy's words: pad symmetrically by k // 2, stack the k shifted copies, sort, take the middle."""
    h, n = k // 2, X.shape[axis]
    pad = [(0, 0), (0, 0)]
    pad[axis] = (h, h)
    P = np.pad(X, pad, mode="symmetric")
    stack = np.stack([np.take(P, np.arange(s, s + n), axis=axis) for s in range(k)])
    return np.sort(stack, axis=0)[h]


@pytest.mark.parametrize("k", [1, 3, 5, 17, 31, 63])
def test_medians_equal_pad_stack_sort_element_for_element(k):
    for i, (F, D) in enumerate(SHAPES):
        X = hm.rows(F, D, seed=100 + i)
        for axis in (0, 1):
            assert np.array_equal(hm.median(X, k, axis), pad_sort_median(X, k, axis)), (F, D, k, axis)


def test_reflect_is_numpy_pad_symmetric_however_often():
    for n in (1, 2, 3, 7):
        base = np.arange(n)
        want = np.pad(base, (40, 40), mode="symmetric")
        assert np.array_equal(hm.reflect(np.arange(-40, n + 40), n), want), n


@pytest.mark.parametrize("k", [1, 3, 5, 17, 31, 63])
def test_medians_equal_scipy_median_filter_where_scipy_still_reflects(k):
    """scipy.ndimage.median_filter(mode="reflect") is the filter librosa calls, and it agrees with the model wherever it reflects.
    Only where k // 2 <= 2 n for the filtered axis of length n: beyond about four periods (k // 2 >= 4 n, e.g. n = 2 and k >= 17,
    and every one-dimensional call with a wide window; seen on scipy 1.15.3) scipy stops reflecting and returns other values, even
    zeros. There the numpy.pad definition of the test above is the contract, and scipy is not asked."""
    ndimage = pytest.importorskip("scipy.ndimage")
    checked = 0
    for i, (F, D) in enumerate(SHAPES):
        X = hm.rows(F, D, seed=200 + i)
        for axis, size in ((0, (k, 1)), (1, (1, k))):
            if k // 2 > 2 * X.shape[axis]:
                continue
            assert np.array_equal(hm.median(X, k, axis), ndimage.median_filter(X, size=size, mode="reflect")), (F, D, k, axis)
            checked += 1
    assert checked


def librosa_softmask(X, X_ref, power, split_zeros):
    """librosa.util.softmask in its own words (librosa 0.10, util/utils.py), on float64 arrays with float32's tiny."""
    if power == np.inf:
        return (X > X_ref).astype(np.float64)
    Z = np.maximum(X, X_ref)
    bad_idx = Z < np.finfo(np.float32).tiny
    Z[bad_idx] = 1
    mask = (X / Z) ** power
    ref_mask = (X_ref / Z) ** power
    good_idx = ~bad_idx
    mask[good_idx] /= mask[good_idx] + ref_mask[good_idx]
    if split_zeros:
        mask[bad_idx] = 0.5
    else:
        mask[bad_idx] = 0.0
    return mask


@pytest.mark.parametrize("margin", hm.MARGINS)
@pytest.mark.parametrize("power", hm.POWERS + [3.0])
def test_masks_and_components_equal_librosas_expressions(power, margin):
    X = hm.rows(40, 33, seed=7)
    kh, kp = 5, 17
    H, P = pad_sort_median(X, kh, 0).astype(np.float64), pad_sort_median(X, kp, 1).astype(np.float64)
    split = margin[0] == 1 and margin[1] == 1
    want = dict(harmonic=librosa_softmask(H.copy(), P * margin[0], power, split), percussive=librosa_softmask(P.copy(), H * margin[1], power, split))
    zeros = 0
    for comp in hm.COMPONENTS:
        kw = dict(component=comp, kernel_size=(kh, kp), power=power, margin=margin)
        assert np.array_equal(hm.hpss64(X, output="mask", **kw), want[comp])
        assert np.array_equal(hm.hpss64(X, **kw), X.astype(np.float64) * want[comp])
        assert np.array_equal(hm.hpss64(X, output="median", **kw), H if comp == "harmonic" else P)
        zeros += int((np.maximum(H, P) < hm.TINY).sum())
    assert zeros  # the rows do run the FLT_MIN branch
    if np.isfinite(power) and split:  # librosa's own invariant: with margins of 1 the two soft masks add up to 1
        assert np.allclose(want["harmonic"] + want["percussive"], 1.0, rtol=0, atol=1e-15)


def test_a_nan_poisons_exactly_its_windows_in_the_model():
    X = hm.rows(40, 33, seed=3)
    X[20, 10] = np.nan
    H, P = hm.median(X, 5, 0), hm.median(X, 7, 1)
    wantH, wantP = np.zeros(X.shape, bool), np.zeros(X.shape, bool)
    wantH[18:23, 10] = True
    wantP[20, 7:14] = True
    assert np.array_equal(np.isnan(H), wantH) and np.array_equal(np.isnan(P), wantP)
    Y = hm.hpss(X, kernel_size=(5, 7))
    assert np.array_equal(np.isnan(Y), wantH | wantP)
    X[20, 10] = np.inf  # an Inf sorts as a number: it is the median of no window here
    assert np.isfinite(hm.median(X, 5, 0)).all() and np.isfinite(hm.median(X, 7, 1)).all()


BAD = [dict(hpss="both"), dict(hpss=True), dict(hpss=1), dict(hpss_kernel_size=0), dict(hpss_kernel_size=30), dict(hpss_kernel_size=65),
       dict(hpss_kernel_size=-3), dict(hpss_kernel_size=31.0), dict(hpss_kernel_size=(31, 32)), dict(hpss_kernel_size=(0, 31)),
       dict(hpss_kernel_size=(31, 31, 31)), dict(hpss_kernel_size=True), dict(hpss_power=0.0), dict(hpss_power=-1.0),
       dict(hpss_power=float("nan")), dict(hpss_power=-float("inf")), dict(hpss_power="2"), dict(hpss_power=True),
       dict(hpss_margin=0.5), dict(hpss_margin=(1.0, 0.99)), dict(hpss_margin=float("inf")), dict(hpss_margin=float("nan")),
       dict(hpss_margin=(1.0,)), dict(hpss_margin="1"), dict(hpss_output="residual"), dict(hpss_output=None), dict(hpss_output=2),
       dict(kind="log_mel"), dict(kind="mel_db"), dict(kind="mfcc"), dict(kind="lin_db"), dict(kind="stft"), dict(kind="chroma"),
       dict(kind="tonnetz"), dict(pcen=True, hpss_output="mask"), dict(pcen=True, hpss_output="median")]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join("%s=%r" % it for it in kw.items()))
def test_bad_keywords_raise_before_the_library_loads(kw, monkeypatch):
    def no_load():
        raise AssertionError("library loaded before the arguments were checked")
    monkeypatch.setattr(spectral, "_load", no_load)
    args = dict(dict(kind="mel_power", hpss="harmonic", n_fft=64, hop_length=16, n_mels=8, n_mfcc=4), **kw)
    with pytest.raises(spectral.SpectralError):
        spectral.get_spectral_batch([b"OggS"], **args)
    with pytest.raises(spectral.SpectralError):
        spectral.get_spectral_from_raw_bytes(b"OggS", **args)


def test_the_arguments_are_checked_with_the_stage_off_and_good_ones_reach_the_library(monkeypatch):
    class Reached(Exception):
        pass

    def no_load():
        raise Reached()
    monkeypatch.setattr(spectral, "_load", no_load)
    for kw in (dict(hpss_kernel_size=30), dict(hpss_power=0), dict(hpss_margin=0.5), dict(hpss_output="x")):
        with pytest.raises(spectral.SpectralError):
            spectral.get_spectral_batch([b"OggS"], kind="log_mel", **kw)  # hpss=None
    with pytest.raises(spectral.SpectralError) as ei:
        spectral.get_spectral_batch([b"OggS"], kind="log_mel", hpss="harmonic")
    assert "log_mel" in str(ei.value) and "mel_power" in str(ei.value)
    for kind in ("mel_power", "lin_power"):
        for comp in hm.COMPONENTS:
            with pytest.raises(Reached):
                spectral.get_spectral_batch([b"OggS"], kind=kind, hpss=comp, hpss_kernel_size=(63, 1), hpss_power=np.inf, hpss_margin=(1, 3.5),
                                            hpss_output="mask")
    with pytest.raises(Reached):
        spectral.get_spectral_batch([b"OggS"], kind="mel_power", hpss="percussive", pcen=True, delta=1)
    with pytest.raises(Reached):  # off: any kind, as before
        spectral.get_spectral_batch([b"OggS"], kind="log_mel")
    with pytest.raises(spectral.SpectralError):  # the linear kinds still refuse the post stage
        spectral.get_spectral_batch([b"OggS"], kind="lin_power", hpss="harmonic", delta=1)


def test_hpss_none_leaves_the_spectral_spec_the_kinds_and_the_dims_alone():
    assert spectral.KINDS == {"mel_power": 1, "log_mel": 2, "mel_db": 3, "mfcc": 4, "lin_power": 5, "lin_db": 6, "stft": 7}
    assert spectral.HPSS_KINDS == ("mel_power", "lin_power")
    s = spectral.spectral_spec("mel_power", n_fft=512, hop_length=128, n_mels=40)
    assert (s.kind, s.n_fft, s.hop_length, s.n_mels) == (1, 512, 128, 40) and spectral.spec_dim(s) == 40
    assert spectral.spec_dim(spectral.spectral_spec("lin_power", n_fft=2048)) == 1025
    from parseoggvorbis_amd import binding
    assert ctypes.sizeof(binding.SpectralSpec) == 72  # unchanged by this stage


def test_hpss_spec_encoding_and_layout():
    from parseoggvorbis_amd import binding
    assert ctypes.sizeof(binding.SpectralHpss) == 40
    names = ["kh", "kp", "component", "output", "power", "margin_h", "margin_p"]
    assert [f[0] for f in binding.SpectralHpss._fields_] == names
    assert [getattr(binding.SpectralHpss, n).offset for n in names] == [0, 4, 8, 12, 16, 24, 32]
    p = spectral.hpss_spec()
    assert [getattr(p, n) for n in names] == [31, 31, 0, 0, 2.0, 1.0, 1.0]
    p = spectral.hpss_spec("percussive", (5, 17), np.inf, (2, 3.5), "median")
    assert [getattr(p, n) for n in names] == [5, 17, 1, 2, np.inf, 2.0, 3.5]
    assert spectral.hpss_spec(kernel_size=np.int64(63), power=np.float32(0.5), output="mask").output == 1


def test_symbols_are_declared_exported_and_in_the_header():
    from parseoggvorbis_amd import binding
    lib = binding.load()
    header = open(os.path.join(ROOT, "include", "vorbis_synth_hip.h")).read()
    assert "HPSS" in header and "typedef struct vsyn_spectral_hpss { /* 40 bytes */" in header
    for s in SYMBOLS:
        assert s in binding.declared_symbols() and hasattr(lib, s)
        assert s + "(" in header, s
    assert lib.vsyn_abi_version() == 5
    host = ctypes.CDLL(spectral.HOST_LIB_PATH)
    assert hasattr(host, "ogg_vorbis_spectral_corpus_hpss")
    assert hasattr(binding.Synth, "spectral_hpss_device")
