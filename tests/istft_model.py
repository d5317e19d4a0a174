"""Float64 model and per-sample error bound of the inverse STFT (include/vorbis_synth_hip.h, "inverse STFT").

Model, fed the device's own float32 rows X [F][n_fft / 2 + 1] (complex64), float32 mask m (optional) and float32 window w
(tests/spectral_lin_model.window32): Y = double(m) * double(X), exact; x_f = numpy.fft.irfft(Y_f, n_fft) in float64 (the imaginary
parts of bins 0 and n_fft / 2 are not read); v_f[j] = w[j] x_f[j] on the window's support; y[t] = (sum_f v_f[t + pad - f hop]) /
W[t], W[t] = sum_f w[t + pad - f hop]^2, over the frames whose support holds t; undivided where W[t] <= FLT_MIN; 0 where no frame
covers t; cut or zero-filled to `length`.

Bound, per sample. u = 2^-24. For frame f let A_f = (1 / n_fft) sum_k c_k (|Re Y_k| + |Im Y_k|), c_k = 2 for 0 < k < n_fft / 2 and
1 for the two end bins: what |x_f[j]| can be at most, whatever j.

  mask product     each component of Y is one float32 product, off by at most u times itself: u A_f on x_f[j]. Without a mask, 0.
  butterflies      K u A_f, K = 4 (log2 n_fft + 2), the count of tests/spectral_lin_model.py read backwards: a butterfly a + w b
                   with a rounded twiddle errs by at most 4 u (|a| + |b|) per component, the operands of a level sum to at most
                   n_fft A_f for any one output, and the device runs the tangling pass (a butterfly with a sum in front: two
                   levels), log2(n_fft / 2) radix-2 levels, and one more level's worth for the second-order terms. The final
                   1 / n_fft is a power of two and exact.
  underflow        a float32 result below FLT_MIN is off by up to 2^-150 instead of u times itself: (K + 2) 2^-150 per frame.
  So |dx_f[j]| <= e_f = (K + [mask]) u A_f + (K + 2) 2^-150.
  window product   v = w x is one float32 product: |dv_f[j]| <= w[j] (e_f + u (|x_f[j]| + e_f)) + 2^-150.
  sum over frames  the device adds the covering frames' v in float64: its own error is below 2^-52 times the number of terms times
                   sum |v|, which is added; the bound of the sum is the sum of the |dv_f| (each already weighted by its w).
  division         all of it divided by W[t] where W[t] > FLT_MIN (W is a float64 sum of exact squares: 2^-50 |y| covers it and
                   the quotient's rounding), else left as it is, as the value is.
  final rounding   u (|y| + bound), plus 2^-150.

Every sample has a bound; one with a small W[t] has a wide one, none is exempt.
"""
import numpy as np

from tests import spectral_lin_model as lm
from tests import spectral_model as sm

U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
DEN = 2.0 ** -150

# (n_fft, hop_length, win_length, center): the framings of the issue's table; the last two are the ones that have samples with
# W <= FLT_MIN (the `tiny` rule) and samples that no frame covers (gaps between frames).
FRAMINGS = [
    (16, 7, 16, True),
    (1024, 256, 700, True),
    (2048, 512, 2048, True),
    (8192, 2048, 8192, True),
    (64, 1, 64, False),
    (512, 700, 400, True),
]


def fid(e):
    return "n%d_h%d_w%d_%s" % (e[0], e[1], e[2], "c" if e[3] else "nc")


def K(n_fft):
    return 4.0 * (np.log2(n_fft) + 2.0)


def num_samples(F, n_fft, hop_length, center):
    if F == 0:
        return 0
    return hop_length * (F - 1) + (0 if center else n_fft)


def _bins(X, mask):
    """Y in float64 (exact products), the imaginary parts of the two end bins dropped."""
    Y = np.asarray(X).astype(np.complex128)
    if mask is not None:
        Y = Y * np.asarray(mask, np.float64)
    Y = Y.copy()
    if Y.shape[0]:
        Y[:, 0] = Y[:, 0].real
        Y[:, -1] = Y[:, -1].real
    return Y


def overlap_add(v, w, n_fft, hop_length, win_length, center, length, dv=None):
    """(y, W, cover [length]; and the bound's sum when dv [F][n_fft] is given): the float64 overlap-add of frames v [F][n_fft] (any
    float dtype; added in float64, ascending f) under window w, over each frame's window support only."""
    F = v.shape[0]
    sup = np.flatnonzero(sm.support(n_fft, win_length))
    pad = n_fft // 2 if center else 0
    full = max(length, num_samples(F, n_fft, hop_length, center)) + 2 * n_fft
    acc, W, cov, db = np.zeros(full), np.zeros(full), np.zeros(full, np.int64), np.zeros(full)
    w64 = np.asarray(w, np.float64)
    for f in range(F):  # ascending f: the device's order
        idx = f * hop_length + sup
        acc[idx] += v[f, sup].astype(np.float64)
        W[idx] += w64[sup] * w64[sup]
        cov[idx] += 1
        if dv is not None:
            db[idx] += dv[f, sup]
    s = slice(pad, pad + length)
    acc, W, cov, db = acc[s], W[s], cov[s], db[s]
    div = W > FLT_MIN
    y = np.where(div, acc / np.where(div, W, 1.0), acc)
    return y, W, cov, np.where(div, db / np.where(div, W, 1.0), db)


def istft(X, n_fft, hop_length, win_length=None, center=True, length=None, mask=None):
    """(y [length] float64, bound [length]): the model and the bound on every sample of the device's float32 output."""
    win_length = n_fft if win_length is None else win_length
    X = np.asarray(X).reshape(-1, n_fft // 2 + 1)
    F = X.shape[0]
    length = num_samples(F, n_fft, hop_length, center) if length is None else length
    w = lm.window32(n_fft, win_length).astype(np.float64)
    Y = _bins(X, mask)
    x = np.fft.irfft(Y, n_fft, axis=1) if F else np.zeros((0, n_fft))
    c = np.full(n_fft // 2 + 1, 2.0)
    c[0] = c[-1] = 1.0
    A = ((np.abs(Y.real) + np.abs(Y.imag)) * c[None, :]).sum(axis=1) / n_fft
    e = (K(n_fft) + (0.0 if mask is None else 1.0)) * U * A + (K(n_fft) + 2.0) * DEN
    v = x * w[None, :]
    dv = w[None, :] * (e[:, None] + U * (np.abs(x) + e[:, None])) + DEN
    dv = dv + 2.0 ** -52 * np.ceil(n_fft / hop_length) * np.abs(v)  # the float64 additions
    y, W, cov, b = overlap_add(v, w, n_fft, hop_length, win_length, center, length, dv)
    b = b + 2.0 ** -50 * np.abs(y)
    return y, b + U * (np.abs(y) + b) + DEN


def check(got, X, n_fft, hop_length, win_length=None, center=True, length=None, mask=None, extra=None, what=""):
    """Asserts that got (the device's float32 samples of one segment) is within the bound of the model, every sample. extra
    [length] (optional): a bound from elsewhere, added (the forward transform's in a round trip). Returns the worst |d| / bound."""
    y, b = istft(X, n_fft, hop_length, win_length, center, length, mask)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == y.shape, (what, got.dtype, got.shape, y.shape)
    if not y.size:
        return 0.0
    if extra is not None:
        b = b + extra
    d = np.abs(got.astype(np.float64) - y)
    ok = np.isfinite(d) & (d <= b)
    assert ok.all(), (what, int((~ok).sum()), np.flatnonzero(~ok)[:4], float(np.nanmax(d / b)))
    return float((d / b).max())


def frames_f32(X, n_fft, win_length=None, mask=None):
    """The frame kernel restated in float32 numpy, operation for operation: X [F][NB] complex64 (and mask [F][NB] float32) ->
    v [F][n_fft] float32, 0 outside the window's support. Tangling pass, log2(n_fft / 2) Stockham passes with conjugated twiddles,
    the 1 / n_fft and the window product."""
    assert lm.is_pow2(n_fft)
    win_length = n_fft if win_length is None else win_length
    X = np.asarray(X, np.complex64).reshape(-1, n_fft // 2 + 1)
    M, h = n_fft // 2, n_fft // 4
    c, s = lm.twiddles32(n_fft)
    xr, xi = X.real.astype(np.float32), X.imag.astype(np.float32)
    if mask is not None:
        m = np.asarray(mask, np.float32)
        xr, xi = m * xr, m * xi
    k = np.arange(M)
    old = np.seterr(invalid="ignore", over="ignore")  # non-finite inputs flow through as on the device
    ar, ai, br, bi = xr[:, k], xi[:, k].copy(), xr[:, M - k], xi[:, M - k].copy()
    ai[:, 0] = 0.0
    bi[:, 0] = 0.0
    er, ei, dr, di = ar + br, ai - bi, ar - br, ai + bi
    wc, ws = c[k][None, :], s[k][None, :]
    re = er - (wc * di + ws * dr)
    im = ei + (wc * dr - ws * di)
    j = np.arange(h)
    Ns = 1
    while Ns < M:
        kk = j & (Ns - 1)
        wc, ws = c[kk * (n_fft // (2 * Ns))][None, :], s[kk * (n_fft // (2 * Ns))][None, :]
        ar, ai, br, bi = re[:, :h], im[:, :h], re[:, h:], im[:, h:]
        tr = wc * br - ws * bi
        ti = wc * bi + ws * br
        j0 = ((j - kk) << 1) + kk
        nre, nim = np.empty_like(re), np.empty_like(im)
        nre[:, j0], nre[:, j0 + Ns] = ar + tr, ar - tr
        nim[:, j0], nim[:, j0 + Ns] = ai + ti, ai - ti
        re, im = nre, nim
        Ns *= 2
    inv = np.float32(1.0 / n_fft)
    x = np.empty((X.shape[0], n_fft), np.float32)
    x[:, 0::2], x[:, 1::2] = re * inv, im * inv
    v = lm.window32(n_fft, win_length)[None, :] * x
    v[:, ~sm.support(n_fft, win_length)] = 0.0
    np.seterr(**old)
    assert v.dtype == np.float32
    return v


def istft_f32(X, n_fft, hop_length, win_length=None, center=True, length=None, mask=None):
    """The device's whole stage restated: frames_f32, then the overlap-add in float64 and one rounding to float32."""
    win_length = n_fft if win_length is None else win_length
    v = frames_f32(X, n_fft, win_length, mask)
    length = num_samples(v.shape[0], n_fft, hop_length, center) if length is None else length
    with np.errstate(invalid="ignore", over="ignore"):
        return overlap_add(v, lm.window32(n_fft, win_length), n_fft, hop_length, win_length, center, length)[0].astype(np.float32)


def random_rows(rng, F, n_fft):
    """F rows of random complex64 bins (no valid STFT: the end bins have imaginary parts too)."""
    nb = n_fft // 2 + 1
    return (rng.standard_normal((F, nb)) + 1j * rng.standard_normal((F, nb))).astype(np.complex64)
