"""The float64 model of the phase vocoder (tests/pv_model.py) without a GPU: against a literal transcription of librosa's sequential
loop, the two host size functions against numpy and Python, rate 1, a stretched and a pitch-shifted bin-centred sine, and the
signed zeros."""
import numpy as np
import pytest

from tests import pv_model as pm

RATES = [0.25, 0.5, 0.8, 1.0, 1.25, 2.0 ** (-2.0 / 12.0), 3.0, 200.0]


@pytest.fixture(scope="module")
def lib():
    from parseoggvorbis_amd import binding
    return binding.load()


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("n_fft,hop,F", [(16, 4, 158), (64, 16, 130), (256, 64, 65)])
def test_model_against_the_sequential_loop(n_fft, hop, F, rate):
    """Only the order of the float64 sum differs (and abs against sqrt): the difference stays within reorder_bound."""
    X = pm.random_rows(np.random.default_rng(n_fft + F), F, n_fft)
    re, im, (m, phi) = pm.vocoder(X, rate, n_fft, hop)
    ref = pm.librosa_loop(X, rate, n_fft, hop)
    assert ref.shape == re.shape and re.shape[0] == len(np.arange(0, F, rate))
    b = pm.reorder_bound(re.shape[0], m, phi)
    d = np.maximum(np.abs(re - ref.real), np.abs(im - ref.imag))
    assert (d <= b).all(), float((d / b).max())
    print("pv model vs loop %u/%u F %u rate %g: worst |d| / bound %.3g, worst relative %.3g" % (n_fft, hop, F, rate, float((d / b).max()),
                                                                                              float((d / np.maximum(m, 1e-300)).max())))


def test_size_functions(lib):
    for rate in RATES + [2.0, 1.0 / 3.0, 0.1, 7.5]:
        for n in range(0, 301):
            assert lib.vsyn_pv_num_rows(n, rate) == len(np.arange(0, n, rate)) == pm.num_rows(n, rate), (n, rate)
            assert lib.vsyn_stretch_num_samples(n, rate) == int(round(n / rate)) == pm.num_samples(n, rate), (n, rate)
    assert lib.vsyn_stretch_num_samples(5, 2.0) == 2 and lib.vsyn_stretch_num_samples(7, 2.0) == 4 and lib.vsyn_stretch_num_samples(1, 2.0) == 0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.vsyn_pv_num_rows(10, bad) == 0 and lib.vsyn_stretch_num_samples(10, bad) == 0


@pytest.mark.parametrize("n_fft,hop", [(16, 4), (1024, 256)])
def test_rate_one_returns_the_rows(n_fft, hop):
    """At rate 1 alpha is 0 and acc_t is A[t] up to whole turns and the accumulated error: the rows come back within the bound."""
    X = pm.random_rows(np.random.default_rng(5), 130, n_fft)
    re, im, (m, phi) = pm.vocoder(X, 1.0, n_fft, hop)
    b = pm.bound(re, m, phi)
    assert (np.abs(re - X.real) <= b).all() and (np.abs(im - X.imag) <= b).all()


# ---- a float64 STFT / inverse STFT pair (periodic Hann, centred, reflect padding) for the stretch of a sine ----
def _hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def _stft(y, n, hop):
    yp = np.pad(np.asarray(y, np.float64), n // 2, mode="reflect")
    F = 1 + (len(yp) - n) // hop
    w = _hann(n)
    return np.stack([np.fft.rfft(w * yp[f * hop:f * hop + n]) for f in range(F)])


def _istft(X, n, hop, length):
    w = _hann(n)
    F = X.shape[0]
    y, W = np.zeros(n + hop * (F - 1)), np.zeros(n + hop * (F - 1))
    for f in range(F):
        y[f * hop:f * hop + n] += w * np.fft.irfft(X[f], n)
        W[f * hop:f * hop + n] += w * w
    y = np.where(W > 1e-30, y / np.maximum(W, 1e-30), y)[n // 2:]
    out = np.zeros(length)
    out[:min(length, len(y))] = y[:length]
    return out


def _stretch(y, rate, n, hop):
    X = _stft(y, n, hop).astype(np.complex64)
    re, im, _ = pm.vocoder(X, rate, n, hop)
    return _istft(re + 1j * im, n, hop, pm.num_samples(len(y), rate))


def _peak_hz(y, sr):
    mid = y[len(y) // 2 - 1024:len(y) // 2 + 1024]
    return float(np.argmax(np.abs(np.fft.rfft(mid * _hann(2048))))) * sr / 2048.0


SR, T, N, HOP, F0 = 8000, 8000, 256, 64, 625.0


@pytest.mark.parametrize("rate", [0.8, 1.25])
def test_stretched_sine_keeps_its_bin(rate):
    y = np.sin(2.0 * np.pi * F0 * np.arange(T) / SR)
    out = _stretch(y, rate, N, HOP)
    assert len(out) == int(round(T / rate))
    assert _peak_hz(out, SR) == _peak_hz(y, SR) == F0


def _resample(y, r_in, r_out):
    """Band-limited resampling in float64 (windowed sinc at the output instants): the test's own, good to far below a bin width."""
    n_out = int(np.ceil(len(y) * r_out / r_in))
    t = np.arange(n_out) * (r_in / r_out)
    cut = min(1.0, r_out / r_in)
    out = np.zeros(n_out)
    half = 32
    base = np.floor(t).astype(np.int64)
    for j in range(-half + 1, half + 1):
        idx = base + j
        x = (t - idx) * cut
        w = np.where(np.abs(t - idx) < half, 0.5 + 0.5 * np.cos(np.pi * (t - idx) / half), 0.0)
        ok = (idx >= 0) & (idx < len(y))
        out += np.where(ok, y[np.clip(idx, 0, len(y) - 1)], 0.0) * cut * np.sinc(x) * w
    return out


@pytest.mark.parametrize("steps", [3, -2])
def test_pitch_shifted_sine(steps):
    """The stage's recipe: rate = 2^(-steps / 12), the stretch, then from rint(sr / rate) Hz to sr, and the length fixed to T."""
    y = np.sin(2.0 * np.pi * F0 * np.arange(T) / SR)
    rate = 2.0 ** (-steps / 12.0)
    from_hz = int(np.rint(SR / rate))
    z = _resample(_stretch(y, rate, N, HOP), from_hz, SR)
    out = np.zeros(T)
    out[:min(T, len(z))] = z[:T]
    assert len(out) == T
    assert abs(_peak_hz(out, SR) - F0 * 2.0 ** (steps / 12.0)) <= SR / 2048.0


def test_signed_zeros_and_a_silent_middle():
    z = np.array([complex(-0.0, 0.0), complex(-0.0, -0.0), complex(0.0, 0.0), complex(0.0, -0.0)], np.complex64)
    A, G = pm.polar(z[None, :])
    want = np.arctan2(np.array([0.0, -0.0, 0.0, -0.0]), np.array([-0.0, -0.0, 0.0, 0.0]))
    assert np.array_equal(A[0], want) and np.array_equal(np.signbit(A[0]), np.signbit(want))
    assert A[0, 0] == np.pi and A[0, 1] == -np.pi and not G.any()
    # rows 3..6 exact zeros of mixed signs: the rows behind them carry the phase the model accumulates through them, whatever the
    # zeros' signs make of the four angles, and every sign pattern is a different, reproducible continuation
    n_fft, hop, F = 16, 4, 12
    rng = np.random.default_rng(3)
    X = pm.random_rows(rng, F, n_fft)
    nb = n_fft // 2 + 1
    outs = []
    for pat in range(2):
        Xz = X.copy()
        for f in range(3, 7):
            Xz[f] = z[(np.arange(nb) + f + pat) % 4]
        re, im, (m, phi) = pm.vocoder(Xz, 1.0, n_fft, hop)
        assert not re[3:7].any() and not im[3:7].any()
        ref = pm.librosa_loop(Xz, 1.0, n_fft, hop)
        b = pm.reorder_bound(F, m, phi)
        assert (np.abs(re - ref.real) <= b).all() and (np.abs(im - ref.imag) <= b).all()
        assert np.abs(re[7:]).min() > 0.0
        outs.append(re)
    assert np.array_equal(outs[0][:3], outs[1][:3])
