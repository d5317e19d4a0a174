"""The inverse-STFT model (tests/istft_model.py) against torch.istft and a direct inverse DFT, its float32 restatement of the device's
operation order against its own bound, and the rules of the header ("inverse STFT") that need no GPU: the `tiny` rule, uncovered
samples and `length`."""
import numpy as np
import pytest

from tests import istft_model as im
from tests import spectral_lin_model as lm
from tests import spectral_model as sm


def _forward(y, n, hop, win, center):
    """The float64 forward STFT of mono y under the float32 window, as complex128 rows."""
    return lm.stft(np.asarray(y, np.float64), n, hop, win, center)[0]


@pytest.mark.parametrize("entry", [e for e in im.FRAMINGS if e[3] and e[1] < e[2]], ids=im.fid)
def test_model_equals_torch_istft(entry):
    """float64, center=True, length=T, on the framings with full overlap; random rows, not a valid STFT."""
    import torch
    n, hop, win, center = entry
    rng = np.random.default_rng(n)
    F = 9
    T = hop * (F - 1) - 3
    X = im.random_rows(rng, F, n).astype(np.complex128)
    w = torch.from_numpy(lm.window32(n, win).astype(np.float64)[(n - win) // 2:(n - win) // 2 + win].copy())
    want = torch.istft(torch.from_numpy(X.T.copy()), n, hop_length=hop, win_length=win, window=w, center=True, length=T).numpy()
    got, _ = im.istft(X, n, hop, win, True, T)
    assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max())


def test_model_equals_a_direct_inverse_dft():
    """n_fft = 16: x[j] = (1/n) sum_{k<n} Yfull[k] exp(+2 pi i j k / n) over the Hermitian extension, the end bins' imaginary parts
    dropped; then window, overlap-add and division written out sample by sample."""
    n, hop, win, center = 16, 7, 16, True
    rng = np.random.default_rng(1)
    F = 6
    X = im.random_rows(rng, F, n)
    m = rng.random((F, n // 2 + 1)).astype(np.float32)
    Y = X.astype(np.complex128) * m.astype(np.float64)
    w = lm.window32(n, win).astype(np.float64)
    T = hop * (F - 1)
    num, den = np.zeros(T + 2 * n), np.zeros(T + 2 * n)
    for f in range(F):
        full = np.zeros(n, np.complex128)
        full[:n // 2 + 1] = Y[f]
        full[0], full[n // 2] = Y[f, 0].real, Y[f, n // 2].real
        full[n // 2 + 1:] = np.conj(Y[f, 1:n // 2][::-1])
        j = np.arange(n)
        x = (full[None, :] * np.exp(2j * np.pi * j[:, None] * j[None, :] / n)).sum(axis=1) / n
        assert np.abs(x.imag).max() < 1e-12
        num[f * hop:f * hop + n] += w * x.real
        den[f * hop:f * hop + n] += w * w
    want = num[n // 2:n // 2 + T] / den[n // 2:n // 2 + T]
    got, _ = im.istft(X, n, hop, win, center, T, mask=m)
    assert np.abs(got - want).max() < 1e-12


@pytest.mark.parametrize("n_fft,hop,win,center", [(16, 7, 16, True), (64, 1, 64, False), (512, 700, 400, True), (2048, 512, 2048, True),
                                                   (8192, 2048, 8192, True)])
@pytest.mark.parametrize("masked", [False, True])
def test_float32_restatement_stays_inside_the_bound(n_fft, hop, win, center, masked):
    """The kernel's operation order in float32 numpy against the float64 model: every sample inside the derived bound."""
    rng = np.random.default_rng(n_fft + masked)
    F = 5 if n_fft >= 2048 else 37
    X = im.random_rows(rng, F, n_fft)
    m = rng.random(X.shape).astype(np.float32) if masked else None
    got = im.istft_f32(X, n_fft, hop, win, center, None, m)
    r = im.check(got, X, n_fft, hop, win, center, None, m, what=("restatement", n_fft, masked))
    print("n_fft %d%s: float32 restatement worst |d| / bound %.3f" % (n_fft, " masked" if masked else "", r))
    assert 0.0 < r <= 1.0


def test_round_trip_of_the_model():
    """forward float64 STFT, then the model inverse: the signal again, on the four fully covered framings, where no sample has
    W <= FLT_MIN (the smallest W stays above 0.4)."""
    for n, hop, win, center in im.FRAMINGS[:4]:
        rng = np.random.default_rng(n)
        T = hop * 11 + hop // 3
        y = rng.standard_normal(T)
        X = _forward(y, n, hop, win, center)
        got, _ = im.istft(X, n, hop, win, center, T)
        assert np.abs(got - y).max() < 1e-10
        v = np.zeros((X.shape[0], n))
        W = im.overlap_add(v, lm.window32(n, win), n, hop, win, center, T)[1]
        assert W.min() > 0.4, (n, W.min())


def test_the_tiny_rule():
    """64 / 1 / 64 uncentred: sample 0 lies under w[0] = 0 of frame 0 alone, W = 0 <= FLT_MIN, and its sum is left undivided (it
    is 0 * x = 0, not 0 / 0); every other sample is divided."""
    n, hop, win, center = im.FRAMINGS[4]
    rng = np.random.default_rng(5)
    F = 40
    X = im.random_rows(rng, F, n)
    T = im.num_samples(F, n, hop, center)
    v = np.zeros((F, n))
    W, cov = im.overlap_add(v, lm.window32(n, win), n, hop, win, center, T)[1:3]
    assert int((W <= im.FLT_MIN).sum()) == 1 and W[0] == 0.0 and cov.min() >= 1
    y, b = im.istft(X, n, hop, win, center, T)
    assert y[0] == 0.0 and np.isfinite(y).all() and np.isfinite(b).all()
    got = im.istft_f32(X, n, hop, win, center, T)
    assert got[0] == 0.0 and np.isfinite(got).all()


def test_uncovered_samples_and_length():
    """512 / 700 / 400 centred over 3000 samples: 1204 samples have W <= FLT_MIN (the gaps between the frames' supports, and the
    zero of the Hann window at each support's first sample); a sample no frame covers is 0; a shorter length cuts, a longer one
    appends zeros."""
    n, hop, win, center = im.FRAMINGS[5]
    T = 3000
    F = sm.num_frames(T, n, hop, center)
    rng = np.random.default_rng(6)
    X = im.random_rows(rng, F, n)
    v = np.zeros((F, n))
    W, cov = im.overlap_add(v, lm.window32(n, win), n, hop, win, center, T)[1:3]
    assert int((W <= im.FLT_MIN).sum()) == 1204
    y, _ = im.istft(X, n, hop, win, center, T)
    assert (cov == 0).any() and (y[cov == 0] == 0.0).all() and (y[cov > 0] != 0.0).sum() > 1000
    short, _ = im.istft(X, n, hop, win, center, 1000)
    assert np.array_equal(short, y[:1000])
    long_, _ = im.istft(X, n, hop, win, center, 9000)
    full = im.num_samples(F, n, hop, center)
    assert np.array_equal(long_[:T], y) and (long_[full + n:] == 0.0).all()
    assert np.array_equal(im.istft_f32(X, n, hop, win, center, 9000)[:1000], im.istft_f32(X, n, hop, win, center, 1000))


def test_nonfinite_footprint_of_the_restatement():
    """A NaN or an Inf in one bin (or its mask) makes exactly the samples under that frame's window support non-finite, w = 0
    included; the imaginary parts of the two end bins are not read."""
    n, hop, win, center = 64, 16, 40, True
    rng = np.random.default_rng(7)
    F = 12
    X = im.random_rows(rng, F, n)
    m = rng.random(X.shape).astype(np.float32)
    T = im.num_samples(F, n, hop, center)
    clean = im.istft_f32(X, n, hop, win, center, T, m)
    woff = (n - win) // 2
    for f, k, val, in_mask in [(0, 3, np.nan, False), (F - 1, 32, np.inf, False), (5, 0, -np.inf, False), (7, 9, np.nan, True), (4, 17, np.inf, True)]:
        X2, m2 = X.copy(), m.copy()
        if in_mask:
            m2[f, k] = val
        else:
            X2[f, k] = complex(val, X[f, k].imag)
        got = im.istft_f32(X2, n, hop, win, center, T, m2)
        t = np.arange(T)
        under = (t + n // 2 - f * hop >= woff) & (t + n // 2 - f * hop < woff + win)
        assert not np.isfinite(got[under]).any(), (f, k, val)
        assert np.array_equal(got[~under], clean[~under]), (f, k, val)
    X2 = X.copy()
    X2[3, 0] = complex(X[3, 0].real, np.nan)
    X2[3, n // 2] = complex(X[3, n // 2].real, np.inf)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(im.istft_f32(X2, n, hop, win, center, T, m), clean)


# ---- get_pcm_batch(hpss=...): the checks run before the library loads ----
BAD_EFFECT = [dict(hpss="residual"), dict(hpss=True), dict(hpss=0), dict(hpss="harmonic", hpss_n_fft=1102), dict(hpss="harmonic", hpss_n_fft=8),
              dict(hpss="harmonic", hpss_n_fft=16384), dict(hpss="harmonic", hpss_n_fft=2048.0), dict(hpss="percussive", hpss_hop_length=0),
              dict(hpss="percussive", hpss_hop_length=1.5), dict(hpss="harmonic", hpss_win_length=4096), dict(hpss="harmonic", hpss_win_length=0),
              dict(hpss="harmonic", hpss_kernel_size=30), dict(hpss="harmonic", hpss_kernel_size=65), dict(hpss="harmonic", hpss_kernel_size=(31, 31, 31)),
              dict(hpss="harmonic", hpss_margin=0.5), dict(hpss="harmonic", hpss_margin=float("nan")), dict(hpss="harmonic", hpss_power=0),
              dict(hpss="harmonic", hpss_power="2")]


def _no_load():
    raise AssertionError("library loaded before the arguments were checked")


@pytest.mark.parametrize("kw", BAD_EFFECT, ids=lambda kw: "-".join("%s=%r" % it for it in kw.items()))
def test_bad_effect_keywords_raise_before_the_library_loads(kw, monkeypatch):
    from parseoggvorbis_amd import pcm
    monkeypatch.setattr(pcm, "_load", _no_load)
    with pytest.raises(pcm.PcmError) as ei:
        pcm.get_pcm_batch([b"OggS"], mono=True, **kw)
    assert "hpss" in str(ei.value)
    with pytest.raises(pcm.PcmError):
        pcm.get_pcm_from_raw_bytes(b"OggS", mono=True, **kw)


def test_the_effect_needs_mono_and_good_keywords_reach_the_library(monkeypatch):
    from parseoggvorbis_amd import pcm

    class Reached(Exception):
        pass

    def reached():
        raise Reached()
    monkeypatch.setattr(pcm, "_load", reached)
    with pytest.raises(pcm.PcmError) as ei:
        pcm.get_pcm_batch([b"OggS"], hpss="harmonic")
    assert "mono=True" in str(ei.value)
    for kw in (dict(hpss="harmonic"), dict(hpss="percussive", hpss_kernel_size=(17, 31), hpss_margin=(1.0, 3.0), hpss_power=np.inf),
               dict(hpss="harmonic", hpss_n_fft=16, hpss_hop_length=3, hpss_win_length=11), dict(hpss="harmonic", hpss_n_fft=8192),
               dict(hpss=None, hpss_n_fft=7, hpss_kernel_size=2)):  # off: its other arguments are not looked at
        with pytest.raises(Reached):
            pcm.get_pcm_batch([b"OggS"], mono=True, sr=16000, trim_db=40.0, loudness_normalize=-23.0, preemphasis=0.97, **kw)
    e = pcm.effect_spec("percussive", (17, 31), 2.0, (1.0, 3.0), 512)
    assert (e.n_fft, e.hop_length, e.win_length, e.hpss.kh, e.hpss.kp, e.hpss.component, e.hpss.output, e.hpss.margin_p) == (512, 128, 512, 17, 31, 1, 0, 3.0)
