"""The constant-Q stage without a GPU: the float64 model (tests/cqt_model.py) against closed forms and against a restatement as a
correlation of the whole signal with each wavelet, the host-only functions of the C ABI (lengths, wavelets, the chroma fold matrix,
the tile) against the model, and every refusal of step 11 on both sides: in Python before the library loads and through the C
functions."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.signal

import __graft_entry__ as entry
from parseoggvorbis_amd import binding, cqt
from tests import cqt_model as m


@pytest.fixture(scope="module")
def lib():
    entry.build_hip()
    return binding.load()


def _tone_plus_noise(T, sr, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(T) / sr
    return 0.3 * np.cos(2 * np.pi * 440.0 * t) + 0.2 * np.cos(2 * np.pi * 1234.5 * t + 1.0) + 0.1 * rng.standard_normal(T)


def hann_image_bound(L, nu):
    """|sum_j w[j] e^(-2 pi i nu j)| / sum_j w[j] for the periodic Hann of L samples at nu cycles per sample: w is three complex
    exponentials (0.5, -0.25, -0.25 at 0 and +-1 / L), each sums to a Dirichlet kernel of modulus at most 1 / |sin(pi x)|, and
    sum_j w[j] = L / 2."""
    d = lambda v: 1.0 / abs(math.sin(math.pi * v))
    return (0.5 * d(nu) + 0.25 * d(nu - 1.0 / L) + 0.25 * d(nu + 1.0 / L)) / (L / 2.0)


def test_a_cosine_at_a_bin_frequency_has_the_closed_form():
    """y = A cos(2 pi f_k t / sr + phi) covering the support: C[t][k] = sqrt(N_k) A / 2 (e^(i ..) + image), the image being the window's
    transform at 2 f_k, bounded analytically; nothing fitted. The issue's prototype value 0.35012 (A = 0.7, sr 8000, fmin 250,
    bpo 3, k = 4) is |C| / sqrt(N_k) of one such frame: inside the same band."""
    A, sr, T = 0.7, 8000, 4000
    sp = m.spec(fmin=250.0, n_bins=9, bins_per_octave=3, hop_length=64)
    N, L, h = m.lengths(sp, sr)
    for k, f in enumerate(m.frequencies(sp)):
        y = A * np.cos(2.0 * np.pi * f * np.arange(T) / sr + 0.3 * k)
        Cx = m.transform(y, sp, sr)
        inside = [t for t in range(Cx.shape[0]) if t * 64 - h[k] >= 0 and t * 64 - h[k] + L[k] <= T]
        assert len(inside) > 20
        image = hann_image_bound(L[k], 2.0 * f / sr)
        assert image < 0.1
        got = np.abs(Cx[inside, k]) / math.sqrt(N[k])
        assert (np.abs(got - A / 2.0) <= (A / 2.0) * image + 1e-12).all(), (k, float(np.abs(got - A / 2.0).max()), image)
        if k == 4:
            assert abs(0.35012 - A / 2.0) <= (A / 2.0) * image
        # scale=False: N_k in place of sqrt(N_k); norm=None: the sum is L_k / 2 times larger
        C2 = m.transform(y, dict(sp, scale=False, norm=None), sr)
        assert np.allclose(np.abs(C2[inside, k]), np.abs(Cx[inside, k]) * math.sqrt(N[k]) * (L[k] / 2.0), rtol=1e-12)


def test_linearity_silence_and_the_shift_by_one_hop():
    """Silence gives zeros and a scaling by a power of two scales every coefficient, both exactly; the transform of a sum is the sum
    of the transforms up to float64 rounding of the sums (2 L eps A); y delayed by hop samples gives the rows delayed by one (the
    frames whose support is clipped at the left edge see the same samples: zeros either way)."""
    sr, hop = 8000, 50
    sp = m.spec(fmin=200.0, n_bins=8, bins_per_octave=4, hop_length=hop)
    y1, y2 = _tone_plus_noise(1500, sr, 1), _tone_plus_noise(1500, sr, 2)
    C1, C2 = m.transform(y1, sp, sr), m.transform(y2, sp, sr)
    assert C1.shape == (1 + 1500 // hop, 8)
    assert not m.transform(np.zeros(1500), sp, sr).any()
    assert np.array_equal(m.transform(0.25 * y1, sp, sr), 0.25 * C1) and np.array_equal(m.transform(-8.0 * y1, sp, sr), -8.0 * C1)
    A = m.transform(np.abs(y1) + np.abs(y2), sp, sr, absolute=True)
    L0 = m.lengths(sp, sr)[1][0]
    assert (np.abs(m.transform(y1 + y2, sp, sr) - (C1 + C2)) <= 2.0 * L0 * 2.0 ** -52 * A + 1e-300).all()
    Cd = m.transform(np.concatenate([np.zeros(hop), y1]), sp, sr)
    assert Cd.shape[0] == C1.shape[0] + 1
    assert (np.abs(Cd[1:] - C1) <= 2.0 * L0 * 2.0 ** -52 * m.transform(np.abs(y1), sp, sr, absolute=True) + 1e-300).all()
    assert m.transform(np.zeros(0), sp, sr).shape == (0, 8) and m.num_frames(sp, 0) == 0 and m.num_frames(sp, 1) == 1


@pytest.mark.parametrize("kw", [dict(), dict(norm=2, scale=False), dict(norm=None, gamma=20.0), dict(tuning=-0.4, filter_scale=1.7)])
def test_model_agrees_with_a_correlation_of_the_whole_signal(kw):
    """An independent route: scipy.signal.fftconvolve of the zero-padded signal with each reversed wavelet, sampled every hop."""
    sr, hop, T = 11025, 97, 2300
    sp = m.spec(fmin=150.0, n_bins=14, bins_per_octave=5, hop_length=hop, **kw)
    y = _tone_plus_noise(T, sr, 3)
    Cx = m.transform(y, sp, sr)
    N, L, h = m.lengths(sp, sr)
    F = m.num_frames(sp, T)
    for k in range(14):
        b, Nk = m.wavelet(sp, sr, k)
        pad = np.concatenate([np.zeros(h[k]), y, np.zeros(L[k] + hop)])
        full = scipy.signal.fftconvolve(pad, b[::-1], mode="valid")  # full[n] = sum_j pad[n + j] b[j]: the frame centred on n
        s = math.sqrt(Nk) if sp["scale"] else Nk
        want = s * full[np.arange(F) * hop]
        scale = s * np.abs(b).sum() * np.abs(y).max()
        assert np.abs(want - Cx[:, k]).max() <= 1e-10 * scale, (k, float(np.abs(want - Cx[:, k]).max()), scale)


def _c(**kw):
    return cqt.cqt_spec(**kw), m.spec(**kw)


LENGTHS = [(8000, dict(fmin=250.0, n_bins=9, bins_per_octave=3), [141, 111, 89, 71, 55, 45, 35, 27, 23]),
           (8000, dict(fmin=100.0, n_bins=5, bins_per_octave=2), [239, 169, 119, 85, 59]),
           (12000, dict(fmin=100.0, n_bins=3, bins_per_octave=1), [200, 100, 50])]


def test_lengths_and_wavelets_of_the_library_are_the_models(lib):
    """N_k BIT-EQUAL as doubles: both sides evaluate the header's expression with the C library's exp2 (cqt_model._exp2 is that
    function) and correctly rounded IEEE operations in the same order, so there is no ulp to allow, and L_k, which hinges on the
    last bit where N_k / 2 is an integer, cannot differ; L_k equal, the expected values of a numpy
    prototype included, and the even L of N_k / 2 an integer (bpo = 1: r = 2, alpha = 3 / 5); the pairs equal to the float32 rounding
    of the model's."""
    for sr, kw, want in LENGTHS:
        sp, msp = _c(**kw)
        rc, N, L = binding.cqt_lengths(sp, sr)
        Nm, Lm, _ = m.lengths(msp, sr)
        assert rc == 0 and list(L) == want == Lm
        assert np.array_equal(N.view(np.uint64), np.array(Nm).view(np.uint64))
        for k in range(msp["n_bins"]):
            got, (b, _) = binding.cqt_basis(sp, sr, k), m.wavelet(msp, sr, k)
            assert np.array_equal(got.real, b.real.astype(np.float32)) and np.array_equal(got.imag, b.imag.astype(np.float32)), (sr, kw, k)
    Nm, Lm, hm = m.lengths(m.spec(fmin=100.0, n_bins=3, bins_per_octave=1), 12000)
    assert Nm[0] == 200.0 and Lm[0] % 2 == 0 and hm[0] == 100  # N_k / 2 an integer: the one way to an even L
    sp, msp = _c()
    rc, N, L = binding.cqt_lengths(sp, 22050)
    assert rc == 0 and L[0] == 11685 and L[83] == 97 and int(L.sum()) == 206580 and list(L) == m.lengths(msp, 22050)[1]
    assert np.array_equal(N.view(np.uint64), np.array(m.lengths(msp, 22050)[0]).view(np.uint64))
    for kw in (dict(norm=2, gamma=13.0, tuning=0.2, filter_scale=0.8), dict(norm=None, scale=False)):
        sp, msp = _c(fmin=300.0, n_bins=7, bins_per_octave=5, **kw)
        rc, N, L = binding.cqt_lengths(sp, 16000)
        assert rc == 0 and list(L) == m.lengths(msp, 16000)[1] and np.array_equal(N.view(np.uint64), np.array(m.lengths(msp, 16000)[0]).view(np.uint64))
        for k in (0, 6):
            got, (b, _) = binding.cqt_basis(sp, 16000, k), m.wavelet(msp, 16000, k)
            assert np.array_equal(got.real, b.real.astype(np.float32)) and np.array_equal(got.imag, b.imag.astype(np.float32))
    assert binding.cqt_tile(sp, 16000)[1] == 1024 and min(binding.cqt_tile(sp, 16000)) >= 1
    assert lib.vsyn_cqt_dim(C.byref(sp)) == 7 and lib.vsyn_cqt_num_frames(C.byref(sp), 1024) == 3 and lib.vsyn_cqt_num_frames(C.byref(sp), 0) == 0
    assert lib.vsyn_cqt_dim(C.byref(_c(output="complex")[0])) == 168 and lib.vsyn_cqt_dim(C.byref(_c(output="tonnetz")[0])) == 6
    assert lib.vsyn_cqt_dim(C.byref(_c(output="chroma", n_chroma=6)[0])) == 6


def numpy_cq_to_chroma(n_input, bins_per_octave, n_chroma, fmin, base_c):
    """librosa.filters.cq_to_chroma's construction, written out."""
    n_merge = bins_per_octave // n_chroma
    M = np.repeat(np.eye(n_chroma), n_merge, axis=1)
    M = np.roll(M, -(n_merge // 2), axis=1)
    n_octaves = int(np.ceil(n_input / bins_per_octave))
    M = np.tile(M, n_octaves)[:, :n_input]
    midi_0 = np.mod(12.0 * (np.log2(fmin) - np.log2(440.0)) + 69.0, 12)
    roll = midi_0 if base_c else midi_0 - 9
    roll = int(np.round(roll * (n_chroma / 12.0)))
    return np.roll(M, roll, axis=0).astype(np.float32)


@pytest.mark.parametrize("bpo,nc", [(12, 12), (36, 12), (24, 12), (36, 36)])
def test_the_fold_matrix_is_numpys_construction(lib, bpo, nc):
    """fmin at C1, A1 and a frequency that is no note, both base_c values, n_bins no multiple of bpo; the model's class list too."""
    for fmin in (m.C1, 55.0, 61.3):
        for base_c in (True, False):
            for nb in (bpo * 2 + 5, 7):
                sp, msp = _c(fmin=fmin, n_bins=nb, bins_per_octave=bpo, output="chroma", n_chroma=nc, base_c=base_c)
                want = numpy_cq_to_chroma(nb, bpo, nc, fmin, base_c)
                got = binding.cq_to_chroma(sp)
                assert got.shape == want.shape == (nc, nb) and np.array_equal(got, want), (fmin, base_c, nb)
                assert list(want.argmax(axis=0)) == m.cq_classes(msp) and (want.sum(axis=0) == 1).all()
    assert binding.cq_to_chroma(_c(output="chroma")[0])[:, 0].argmax() == 0
    assert binding.cq_to_chroma(_c(output="chroma", base_c=False)[0])[:, 0].argmax() == 3  # C1 is row 3 when row 0 is A
    with pytest.raises(binding.VsynError):
        binding.cq_to_chroma(_c()[0])  # not a chroma output


BAD_PY = [dict(n_bins=0), dict(n_bins=257), dict(n_bins=12.0), dict(bins_per_octave=0), dict(bins_per_octave=257), dict(hop_length=0),
          dict(hop_length=True), dict(fmin=0.0), dict(fmin=-3.0), dict(fmin=float("inf")), dict(fmin=float("nan")), dict(fmin="C1"),
          dict(filter_scale=0.0), dict(filter_scale=-1.0), dict(filter_scale=float("inf")), dict(gamma=-0.1), dict(gamma=float("nan")),
          dict(tuning=float("inf")), dict(tuning=None), dict(power=0), dict(power=3), dict(power=1.5), dict(norm=0), dict(norm=3),
          dict(norm=np.inf), dict(scale=1), dict(output="db"), dict(output="chroma"), dict(sr=0), dict(sr=-1), dict(errors="ignore"),
          dict(threads=-1), dict(files_per_submit=0)]
BAD_CHROMA = [dict(n_chroma=0), dict(n_chroma=257), dict(n_chroma=5), dict(n_chroma=24, bins_per_octave=36), dict(chroma_norm=3),
              dict(chroma_norm="max"), dict(base_c=1), dict(tonnetz=1), dict(n_octaves=0), dict(n_octaves=8), dict(bins_per_octave=0),
              dict(output="chroma"), dict(n_bins=84)]
GOOD_PY = [dict(n_bins=1), dict(n_bins=256), dict(bins_per_octave=1), dict(bins_per_octave=256), dict(hop_length=1), dict(fmin=1e-3),
           dict(filter_scale=1e-3), dict(gamma=0.0), dict(tuning=-7.5), dict(power=2), dict(norm=None), dict(norm=2), dict(scale=False),
           dict(output="complex")]


def _no_load():
    raise AssertionError("the library must not be loaded for an invalid argument")


@pytest.mark.parametrize("kw", BAD_PY, ids=[str(k) for k in BAD_PY])
def test_bad_cqt_arguments_are_refused_before_the_library_loads(kw, monkeypatch):
    monkeypatch.setattr(cqt, "_load", _no_load)
    with pytest.raises(cqt.CqtError):
        cqt.get_cqt_batch([b""], **kw)
    with pytest.raises(cqt.CqtError):
        cqt.get_cqt_from_raw_bytes(b"", **kw)


@pytest.mark.parametrize("kw", BAD_CHROMA, ids=[str(k) for k in BAD_CHROMA])
def test_bad_chroma_cqt_arguments_are_refused_before_the_library_loads(kw, monkeypatch):
    monkeypatch.setattr(cqt, "_load", _no_load)
    with pytest.raises((cqt.CqtError, TypeError)):
        cqt.get_chroma_cqt_batch([b""], **kw)
    if "output" not in kw and "n_bins" not in kw:  # (those two are no keywords of this entry: a TypeError)
        with pytest.raises(cqt.CqtError):
            cqt.get_chroma_cqt_batch([b""], **kw)


def test_the_accepted_side_of_every_python_check_reaches_the_library(monkeypatch):
    reached = []
    monkeypatch.setattr(cqt, "_load", lambda: reached.append(1) or _no_load_marker())
    for kw in GOOD_PY:
        with pytest.raises(_Reached):
            cqt.get_cqt_batch([b""], **kw)
    for kw in (dict(n_chroma=1), dict(n_chroma=36), dict(n_octaves=1), dict(chroma_norm=None), dict(base_c=False), dict(tonnetz=True),
               dict(n_octaves=7, bins_per_octave=36), dict(n_chroma=256, bins_per_octave=256, n_octaves=1)):
        with pytest.raises(_Reached):
            cqt.get_chroma_cqt_batch([b""], **kw)
    assert len(reached) == len(GOOD_PY) + 8


class _Reached(Exception):
    pass


def _no_load_marker():
    raise _Reached()


def _raw(**kw):
    d = dict(n_bins=12, bins_per_octave=12, hop_length=64, options=1, output=1, power=1, norm=1, n_chroma=12, chroma_norm=3, reserved=0,
             fmin=200.0, tuning=0.0, filter_scale=1.0, gamma=0.0)
    d.update(kw)
    return binding.CqtSpec(**d)


BAD_C = [dict(n_bins=0), dict(n_bins=257), dict(bins_per_octave=0), dict(bins_per_octave=257), dict(hop_length=0), dict(fmin=0.0),
         dict(fmin=float("inf")), dict(fmin=float("nan")), dict(filter_scale=0.0), dict(filter_scale=float("nan")), dict(gamma=-1e-9),
         dict(gamma=float("inf")), dict(tuning=float("nan")), dict(power=0), dict(power=3), dict(norm=3), dict(output=0), dict(output=5),
         dict(options=4), dict(reserved=1), dict(output=3, n_chroma=0), dict(output=3, n_chroma=257), dict(output=3, n_chroma=5),
         dict(output=4, chroma_norm=4)]
GOOD_C = [dict(n_bins=1), dict(n_bins=256, bins_per_octave=128, fmin=1000.0), dict(bins_per_octave=1, n_bins=3), dict(bins_per_octave=256),
          dict(hop_length=1), dict(fmin=30.0), dict(gamma=0.0), dict(power=2), dict(norm=0), dict(norm=2), dict(output=2),
          dict(options=3), dict(output=3, n_chroma=1), dict(output=3, n_chroma=12, bins_per_octave=36), dict(output=4, chroma_norm=0),
          dict(output=1, n_chroma=999, chroma_norm=99)]


def test_every_check_of_the_c_functions_on_both_sides(lib):
    """vsyn_cqt_dim / vsyn_cqt_num_frames / vsyn_cqt_lengths / vsyn_cqt_tile refuse each invalid spec and accept its neighbour; the
    chroma fields are read for the chroma outputs only."""
    out = np.zeros(3, np.uint32)
    for kw in BAD_C:
        sp = _raw(**kw)
        assert lib.vsyn_cqt_dim(C.byref(sp)) == 0 and lib.vsyn_cqt_num_frames(C.byref(sp), 4096) == 0, kw
        assert lib.vsyn_cqt_lengths(16000, C.byref(sp), None, None) == binding.VSYN_ERR_INVALID, kw
        assert lib.vsyn_cqt_tile(C.byref(sp), 16000, out.ctypes.data) == binding.VSYN_ERR_INVALID, kw
    for kw in GOOD_C:
        sp = _raw(**kw)
        assert lib.vsyn_cqt_dim(C.byref(sp)) > 0 and lib.vsyn_cqt_num_frames(C.byref(sp), 4096) == 1 + 4096 // sp.hop_length, kw
        assert lib.vsyn_cqt_lengths(48000, C.byref(sp), None, None) in (binding.VSYN_OK, binding.VSYN_CQT_RATE_REFUSED), kw
        assert lib.vsyn_cqt_tile(C.byref(sp), 16000, out.ctypes.data) == binding.VSYN_OK, kw
    assert lib.vsyn_cqt_lengths(0, C.byref(_raw()), None, None) == binding.VSYN_ERR_INVALID
    assert lib.vsyn_cqt_dim(None) == 0


def test_the_caps_and_the_rate_rule_on_both_sides_of_their_edges(lib):
    """bpo = 1 with filter_scale = 3 / 5 makes Q = 1 and N_k = sr / f_k exactly: L_0 = 2^17 is accepted and 2^17 + 1 refused; with
    bins a semitone-fraction apart the table sum_k L_k crosses 2^23 between two bin counts the model names; step 10 at the first
    rate that fails it (the model's test, scanned down from an accepted rate)."""
    q1 = dict(bins_per_octave=1, filter_scale=3.0 / 5.0, n_bins=1)
    for L0, want in (((1 << 17) - 1, 0), (1 << 17, 0), ((1 << 17) + 1, 1), ((1 << 17) + 2, 1)):
        kw = dict(q1, fmin=65536.0 / L0)
        sp, msp = _c(**kw)
        assert m.lengths(msp, 65536)[1] == [L0]
        rc, N, L = binding.cqt_lengths(sp, 65536)
        assert rc == want and list(L) == [L0], (L0, rc)
    # the table: 256 bins of about 2^15 samples each; the model finds the last count that fits
    kw = dict(fmin=20.0, bins_per_octave=256, filter_scale=0.1, n_bins=256)
    sr = 48000
    Lm = m.lengths(m.spec(**kw), sr)[1]
    assert Lm[0] <= m.MAX_L0 and sum(Lm) > m.MAX_TABLE
    fits = max(n for n in range(1, 257) if sum(Lm[:n]) <= m.MAX_TABLE)
    assert 1 <= fits < 256
    for nb, want in ((fits, 0), (fits + 1, 1)):
        rc, N, L = binding.cqt_lengths(cqt.cqt_spec(**dict(kw, n_bins=nb)), sr)
        assert rc == want and int(L.astype(np.uint64).sum()) == sum(Lm[:nb]), (nb, rc)
    # step 10
    sp, msp = _c(fmin=110.0, n_bins=48, bins_per_octave=12)
    sr = 8000
    assert not m.rate_refused(msp, sr)
    while not m.rate_refused(msp, sr):
        sr -= 1
    assert binding.cqt_lengths(sp, sr + 1)[0] == binding.VSYN_OK and binding.cqt_lengths(sp, sr)[0] == binding.VSYN_CQT_RATE_REFUSED
    _, Q = m.quality(msp)
    assert m.frequencies(msp)[-1] * (1.0 + 0.5 * 1.50018310546875 / Q) > sr / 2.0
    with pytest.raises(binding.VsynError):
        binding.cqt_basis(sp, sr, 0)
    assert binding.cqt_lengths(sp, sr)[2][0] == m.lengths(msp, sr)[1][0]  # (N and L are filled all the same)


def test_the_bound_is_finite_and_small_where_it_must_be():
    """The bound at L = 2^17 with float32 accumulation stays below 2e-5 of sum |y| |b| s_k (150 roundings), which is what lets the
    kernel run in float32; a silent input has bound 0 and must come out as exact zeros."""
    sp = m.spec(fmin=0.5, n_bins=1, bins_per_octave=1, filter_scale=3.0 / 5.0, hop_length=100000)
    y = np.ones(140000, np.float32)
    want, tol = m.rows(y, sp, 65536, 1024)
    A = m.transform(np.abs(y.astype(np.float64)), sp, 65536, absolute=True)
    assert (tol <= 2e-5 * A).all() and (tol > 0).all()
    want, tol = m.rows(np.zeros(3000, np.float32), m.spec(fmin=200.0, n_bins=8, bins_per_octave=4), 8000, 1024)
    assert not want.any() and not tol.any()
