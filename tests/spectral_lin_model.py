"""Float64 model and per-frame error bound of the linear spectra (include/vorbis_synth_hip.h, "linear spectra").

Model: y = the float64 mean of the channels; v_j = (double)float32(w_j) * y_pad[f hop + j] exactly (w the periodic Hann of
tests/spectral_model.py, rounded to float32 as the device's table is); X = numpy.fft.rfft(v) in float64.

Bound. u = 2^-24, A_f = sum_j |v_j| of frame f. Each of re_k, im_k of the device lies within B_f = K u A_f of the model:

  FFT path (n_fft a power of two), K = 4 (log2 n_fft + 2). To first order a butterfly a + w b with a rounded twiddle errs by at
    most 3 u |b| (twiddle rounding, two products, their sum) + u (|a| + |b|) (the final sum) <= 4 u (|a| + |b|) per component. For
    any one output the operands of a level sum to at most A_f (each level's operands are partial sums of the v_j with unit-modulus
    weights). The device runs log2(n_fft / 2) radix-2 levels and the untangling pass, which is a butterfly with a halving in front
    and counts as two; one more level's worth covers the rounding of w y to float32 and the second-order terms. That is
    (log2 n_fft - 1) + 2 + 1 = log2 n_fft + 2 levels of 4 u A_f.
  Direct path (any other n_fft), K = win_length + 3: a float32 fma chain of win_length terms (term i is followed by
    win_length - i roundings of partial sums, each at most A_f), rounded twiddles, the rounded product w * twiddle and the model's
    own rounding of the window.

  C > 1 channels: the device's float32 downmix is within (C + 1) u (1 / C) sum_c |x_c[t]| of the float64 mean per sample
  (tests/test_gpu_condition.py); weighted by w it adds E_f = sum_j w_j (C + 1) u mean_c |x_c| to B_f. C = 1 is exact.

From B_f (B below includes E_f), with X the model's bin:
  lin_power, power 1: sqrt(2) B + 2 u |X|; power 2: 2 sqrt(2) |X| B + 2 B^2 + 3 u |X|^2; both plus one more float32 rounding
    of the result, u (S + bound).
  lin_db: the image of [S - dS, S + dS] through 10 log10(max(., amin)), widened by the float32 evaluation: log10f is good to 2 ulp
    and the product with 10 rounds once (4 u |D| together, generously), and amin itself is rounded to float32, which moves the
    floor by 10 log10(1 + u) < 2.6e-7 dB (5.2e-7 allowed). The clamp max(D, max_segment D - top_db) is monotone in both arguments,
    so the device's value lies between the clamp of the lower ends and the clamp of the upper ends.
"""
import numpy as np

from tests import spectral_model as sm

U = 2.0 ** -24

# (n_fft, hop_length, win_length, center, T): the framings of the GPU grid (tests/test_gpu_spectral_lin.py) with the signal length
# each is run at; the first five are FFT-path sizes, 1102 and 18 take the direct loop.
GRID = [
    (16, 7, 16, True, 700),
    (64, 1, 64, False, 500),
    (512, 700, 400, True, 6000),
    (2048, 512, 2048, True, 9000),
    (8192, 2048, 8192, True, 20000),
    (1102, 441, 1102, True, 6000),
    (18, 5, 17, False, 400),
    (1024, 256, 700, True, 5000),
]


def signals(T, n_fft, seed=0):
    """The grid's inputs, mono float32 [T]: seeded noise, an off-bin sine plus 1e-4 noise, DC, and a loud burst next to a
    near-silent stretch (the case for the per-frame bound)."""
    rng = np.random.default_rng(seed + n_fft)
    t = np.arange(T, dtype=np.float64)
    noise = 0.3 * rng.standard_normal(T)
    sine = 0.7 * np.sin(2.0 * np.pi * (5.37 / n_fft) * t + 0.3) + 1e-4 * rng.standard_normal(T)
    dc = np.full(T, 0.25)
    burst = 1e-6 * rng.standard_normal(T)
    burst[T // 3:T // 3 + max(n_fft // 2, 8)] += 0.9 * rng.standard_normal(max(n_fft // 2, 8))
    return {k: v.astype(np.float32) for k, v in (("noise", noise), ("sine", sine), ("dc", dc), ("burst", burst))}


def is_pow2(n):
    return n & (n - 1) == 0


def K(n_fft, win_length=None):
    win_length = n_fft if win_length is None else win_length
    return 4.0 * (np.log2(n_fft) + 2.0) if is_pow2(n_fft) else win_length + 3.0


def window32(n_fft, win_length=None):
    return sm.window(n_fft, win_length).astype(np.float32)


def frames(x, n_fft, hop_length, win_length=None, center=True):
    """(v [F][n_fft] float64, E [F]): the windowed frames of planar x[C][T] (or mono [T]) and the downmix term of the bound."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[None, :]
    Cn, T = x.shape
    y = x.mean(axis=0) if Cn > 1 else x[0]
    dmix = (Cn + 1) * U * np.abs(x).mean(axis=0) if Cn > 1 else np.zeros(T)
    F = sm.num_frames(T, n_fft, hop_length, center)
    if F == 0:
        return np.zeros((0, n_fft)), np.zeros(0)
    p = n_fft // 2 if center else 0
    w = window32(n_fft, win_length).astype(np.float64)
    idx = np.arange(F)[:, None] * hop_length + np.arange(n_fft)[None, :]
    v = np.pad(y, (p, p))[idx] * w[None, :]
    v[:, ~sm.support(n_fft, win_length)] = 0.0  # v is 0 outside the window's support whatever the sample there is, an Inf or NaN too
    return v, (np.pad(dmix, (p, p))[idx] * w[None, :]).sum(axis=1)


def stft(x, n_fft, hop_length, win_length=None, center=True, extra=None):
    """(X [F][NB] complex128, B [F]): the model and the bound on each of re, im per frame. extra [T] (optional): a bound on
    |dy| per sample of the mono signal from elsewhere (a PCM difference), added weighted by w."""
    v, E = frames(x, n_fft, hop_length, win_length, center)
    B = K(n_fft, win_length) * U * np.abs(v).sum(axis=1) + E
    if extra is not None and v.shape[0]:
        B = B + frames(np.asarray(extra, np.float64), n_fft, hop_length, win_length, center)[0].sum(axis=1)
    return np.fft.rfft(v, axis=1), B


def power_bound(X, B, power):
    """(S, dS): the model's |X|^power and the bound on the device's float32 value."""
    a = np.abs(X)
    Bc = B[:, None]
    if int(power) == 1:
        S, d = a, np.sqrt(2.0) * Bc + 2.0 * U * a
    else:
        S, d = a * a, 2.0 * np.sqrt(2.0) * a * Bc + 2.0 * Bc * Bc + 3.0 * U * a * a
    return S, d + U * (S + d)


def _db(S, amin):
    return 10.0 * np.log10(np.maximum(S, amin))


def db_interval(S, dS, amin=1e-10, top_db=80.0):
    """(want, lo, hi) of one segment: the model's lin_db rows and the interval that holds the device's."""
    want, lo, hi = _db(S, amin), _db(S - dS, amin), _db(S + dS, amin)
    lo = lo - (4.0 * U * np.abs(lo) + 5.2e-7)
    hi = hi + (4.0 * U * np.abs(hi) + 5.2e-7)
    if top_db and np.isfinite(want).any():  # the maximum is over the finite values (sm.clamp_top_db); lo and hi are NaN where want is
        want = sm.clamp_top_db(want, top_db)
        fin = np.isfinite(want)
        tl, th = lo[fin].max() - top_db, hi[fin].max() - top_db
        lo = np.maximum(lo, tl - U * abs(tl))
        hi = np.maximum(hi, th + U * abs(th))
    return want, lo, hi


def check(got, x, kind, n_fft, hop_length, win_length=None, center=True, power=2, amin=1e-10, top_db=80.0, extra=None, what=""):
    """Asserts that got (the device's rows of one segment; complex64 or interleaved float32 for "stft") is within the bound of the
    model on x, every value. Returns the worst |d| / bound (for "lin_db": the worst position in the interval, 1 = at its end)."""
    X, B = stft(x, n_fft, hop_length, win_length, center, extra)
    nb = n_fft // 2 + 1
    if kind == "stft":
        g = np.asarray(got)
        g = g.view(np.complex64) if g.dtype == np.float32 else g
        assert g.shape == X.shape, (what, g.shape, X.shape)
        if not X.size:
            return 0.0
        g = g.astype(np.complex128)
        d = np.maximum(np.abs(g.real - X.real), np.abs(g.imag - X.imag))
        tol = np.broadcast_to(B[:, None], d.shape)
    else:
        assert got.dtype == np.float32 and got.shape == (X.shape[0], nb), (what, got.shape, X.shape)
        if not X.size:
            return 0.0
        S, dS = power_bound(X, B, power)
        if kind == "lin_power":
            d, tol = np.abs(got.astype(np.float64) - S), dS
        else:
            want, lo, hi = db_interval(S, dS, amin, top_db)
            g = got.astype(np.float64)
            bad = (g < lo) | (g > hi) | ~np.isfinite(g)
            assert not bad.any(), (what, kind, int(bad.sum()), np.argwhere(bad)[:4], g[bad][:4], lo[bad][:4], hi[bad][:4])
            return float(np.max(np.where(g >= want, (g - want) / np.maximum(hi - want, 1e-300), (want - g) / np.maximum(want - lo, 1e-300))))
    ok = np.isfinite(d) & (d <= tol)
    assert ok.all(), (what, kind, int((~ok).sum()), np.argwhere(~ok)[:4], float(np.nanmax(d / np.maximum(tol, 1e-300))))
    nz = tol > 0
    return float((d[nz] / tol[nz]).max()) if nz.any() else 0.0


def twiddles32(n_fft):
    a = 2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft
    return np.cos(a).astype(np.float32), np.sin(a).astype(np.float32)


def fft_f32(v32, n_fft):
    """The device's FFT path restated in float32 numpy, operation for operation: v32 [F][n_fft] float32 (the rounded products
    w * y) -> (re, im) [F][NB] float32. z[m] = v[2m] + i v[2m+1]; log2(M) Stockham radix-2 passes (a = z[j], b = z[j + M/2],
    t = w b, out[j0] = a + t, out[j0 + Ns] = a - t, j0 = 2 (j - k) + k, k = j mod Ns, w = exp(-2 pi i k / (2 Ns))); untangling."""
    assert is_pow2(n_fft) and v32.dtype == np.float32
    M = n_fft // 2
    h = M // 2
    c, s = twiddles32(n_fft)
    re, im = v32[:, 0::2].copy(), v32[:, 1::2].copy()
    j = np.arange(h)
    Ns = 1
    while Ns < M:
        k = j & (Ns - 1)
        wc, ws = c[k * (n_fft // (2 * Ns))][None, :], s[k * (n_fft // (2 * Ns))][None, :]
        ar, ai, br, bi = re[:, :h], im[:, :h], re[:, h:], im[:, h:]
        tr = wc * br + ws * bi
        ti = wc * bi - ws * br
        j0 = ((j - k) << 1) + k
        nre, nim = np.empty_like(re), np.empty_like(im)
        nre[:, j0], nre[:, j0 + Ns] = ar + tr, ar - tr
        nim[:, j0], nim[:, j0 + Ns] = ai + ti, ai - ti
        re, im = nre, nim
        Ns *= 2
    k = np.arange(M)
    ar, ai, br, bi = re[:, k], im[:, k], re[:, (M - k) % M], im[:, (M - k) % M]
    half = np.float32(0.5)
    er, ei, qr, qi = half * (ar + br), half * (ai - bi), half * (ai + bi), half * (br - ar)
    wc, ws = c[k][None, :], s[k][None, :]
    xr = er + (wc * qr + ws * qi)
    xi = ei + (wc * qi - ws * qr)
    return (np.concatenate([xr, (re[:, :1] - im[:, :1])], axis=1).astype(np.float32),
            np.concatenate([xi, np.zeros_like(im[:, :1])], axis=1).astype(np.float32))
