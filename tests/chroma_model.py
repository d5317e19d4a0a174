"""Float64 model and per-frame error bound of the chroma and tonnetz rows (include/vorbis_synth_hip.h, "chroma").

Model: filterbank() is librosa.filters.chroma's recipe with its inner norm=2 as the header writes it, in float64 (filterbank32: cast to
float32 with the flush of magnitudes below FLT_MIN, what the device's table holds). S = |X|^power of tests/spectral_lin_model.py's
float64 STFT; R = W32 S; the row is R / N under the chosen norm unless N < FLT_MIN; tonnetz = phi (row / L1(row)) with the same rule.
A frame with a value of R that is not finite is all NaN. librosa is not among the test dependencies; parity with it is not claimed.

Bound (u = 2^-24), per frame, first-order terms kept with their second-order companions where they are cheap:

  S: dS[k] from spectral_lin_model.power_bound with B_f = K u sum_j |v_j| (K = 4 (log2 n_fft + 2) on the FFT path, win_length + 3 on
     the direct path): the device computes S with the same operations as lin_power.
  R: the device's weight is the float32 rounding of a double that may differ from the model's by an ulp of its libm, and is flushed
     below FLT_MIN: |W_dev - W| <= 2^-23 W + FLT_MIN (the table check of tests/test_chroma_cpu.py). All terms of the sum are >= 0, so
       dR[c] = sum_k W dS + sum_k (2^-23 W + FLT_MIN) (S + dS) + g(m) (R + both)
     with g(m) = m u / (1 - m u) and m the roundings on the longest path of the documented order: a lane's fma chain of
     ceil(bins / 64) terms, 6 levels of the shuffle tree and, on the direct path, one more addition per chunk of 256 bins (bins = NB
     on the FFT path, 256 on the direct path).
  N: L1 and max: |N_dev - N| <= sum resp. max of dR plus, for L1, g(ceil(n_chroma / 64) + 6) of the sum. L2: the 2-norm moves by at
     most the 2-norm of dR; the device evaluates m sqrtf(sum (R / m)^2), m = max |R|: each quotient rounds once (2 u on its square), the
     fma chain and tree add ceil(n_chroma / 64) + 6 roundings to the sum, the root halves the sum's relative error and rounds, the
     product rounds: below g(ceil(n_chroma / 64) + 9) of N in all.
  row = R / N: (dR + |row| dN) / (N - dN) plus u |row| for the correctly rounded division, where dN < N / 2. Where the norm is within
     its own error bound (the S bound is relative to the frame's sum_j |v_j|, not to the bins that carry weight: a DC input's
     magnitude spectrum at a large n_fft), only the range remains: both rows lie in [0, max(1 + 4 u, R + dR)], R being >= 0.
  tonnetz: the second L1 normalisation propagates the same way from the row and its bound; then
     d out[i] = sum_c |phi| du + (u + g(n_chroma)) sum_c |phi| (|u| + du): phi rounded to float32 and one fma chain over c.

The FLT_MIN rule cannot differ between model and device only if no frame has 0 < N < 1e-30: rows() asserts that on every input."""
import functools

import numpy as np

from tests import spectral_lin_model as lm

U = lm.U
FLT_MIN = float(np.finfo(np.float32).tiny)
DBL_MIN = float(np.finfo(np.float64).tiny)
NORMS = {None: 0, 1: 1, 2: 2, np.inf: 3}


def filterbank(sr, n_fft, n_chroma=12, tuning=0.0, ctroct=5.0, octwidth=2.0, base_c=True):
    """W [n_chroma][NB] float64 ("chroma", step 2)."""
    nc = float(n_chroma)
    q = np.empty(n_fft, np.float64)
    a16 = 440.0 * 2.0 ** (tuning / nc) / 16.0
    q[1:] = nc * np.log2((np.arange(1, n_fft, dtype=np.float64) * sr / n_fft) / a16)
    q[0] = q[1] - 1.5 * nc
    bw = np.concatenate([np.maximum(q[1:] - q[:-1], 1.0), [1.0]])
    h = np.round(nc / 2.0)  # ties to even
    D = np.remainder((q[None, :] - np.arange(n_chroma, dtype=np.float64)[:, None]) + h + 10.0 * nc, nc) - h
    W = np.exp(-0.5 * (2.0 * D / bw[None, :]) ** 2)
    nrm = np.sqrt((W * W).sum(axis=0))
    nrm[nrm < DBL_MIN] = 1.0
    W = W / nrm[None, :]
    if octwidth is not None:
        W = W * np.exp(-0.5 * ((q / nc - ctroct) / octwidth) ** 2)[None, :]
    if base_c:
        W = np.roll(W, -3 * (n_chroma // 12), axis=0)
    return np.ascontiguousarray(W[:, :n_fft // 2 + 1])


@functools.lru_cache(maxsize=64)
def filterbank32(sr, n_fft, n_chroma=12, tuning=0.0, ctroct=5.0, octwidth=2.0, base_c=True):
    """The table the device holds: float32, magnitudes below FLT_MIN stored as 0 (cached: leave it unchanged)."""
    W = filterbank(sr, n_fft, n_chroma, tuning, ctroct, octwidth, base_c).astype(np.float32)
    W[np.abs(W) < np.float32(FLT_MIN)] = 0.0
    W.setflags(write=False)
    return W


def phi(n_chroma):
    """[6][n_chroma] float64 ("chroma", step 4)."""
    s = np.array([7 / 6, 7 / 6, 3 / 2, 3 / 2, 2 / 3, 2 / 3])
    o = np.array([0.5, 0.0, 0.5, 0.0, 0.5, 0.0])
    r = np.array([1.0, 1.0, 1.0, 1.0, 0.5, 0.5])
    c = np.arange(n_chroma, dtype=np.float64)
    return r[:, None] * np.cos(np.pi * (s[:, None] * (12.0 * c[None, :] / n_chroma) - o[:, None]))


def _gamma(m):
    return m * U / (1.0 - m * U)


def normalize(R, dR, norm):
    """(row, drow) of rows R [F][n] with bounds dR under norm (0 none, 1 L1, 2 L2, 3 max) and the FLT_MIN rule."""
    if norm == 0:
        return R.copy(), dR.copy()
    n = R.shape[1]
    mc = -(-n // 64)
    a = np.abs(R)
    if norm == 1:
        N = a.sum(axis=1)
        dN = dR.sum(axis=1) + _gamma(mc + 6) * (N + dR.sum(axis=1))
    elif norm == 3:
        N = a.max(axis=1)
        dN = dR.max(axis=1)
    else:
        N = np.sqrt((a * a).sum(axis=1))
        e = np.sqrt((dR * dR).sum(axis=1))  # the 2-norm moves by at most the 2-norm of the change
        dN = e + _gamma(mc + 9) * (N + e)
    assert not ((N > 0.0) & (N < 1e-30)).any(), "a frame with 0 < N < 1e-30: the FLT_MIN rule could differ between model and device"
    assert (R >= 0.0).all()  # (weights and spectra are: the fall-back below uses it)
    live = N >= FLT_MIN
    sure = live & (dN < 0.5 * N)
    Ns = np.where(live, N, 1.0)[:, None]
    row = np.where(live[:, None], R / Ns, R)
    first = (dR + np.abs(row) * dN[:, None]) / (Ns - np.where(sure, dN, 0.0)[:, None]) + U * np.abs(row)
    # a norm within its own error bound (a DC input's magnitude spectrum at a large n_fft): the device's row is R' / N' in [0, 1 + 4 u],
    # or R' <= R + dR itself if its N' fell below FLT_MIN; the model's lies in [0, 1]
    coarse = np.maximum(1.0 + 4.0 * U, R + dR)
    drow = np.where(sure[:, None], first, np.where(live[:, None], coarse, dR))
    return row, drow


def rows(x, kind, sr, n_fft, hop_length, win_length=None, center=True, power=2, n_chroma=12, tuning=0.0, chroma_norm=np.inf, ctroct=5.0,
         octwidth=2.0, base_c=True, extra=None):
    """(want [F][dim], bound [F][dim]) of planar x[C][T] (or mono [T]) for kind "chroma" or "tonnetz"; a frame under the non-finite
    rule is NaN in want (and its bound 0)."""
    with np.errstate(invalid="ignore"):  # (an Inf sample times a window value of 0)
        X, B = lm.stft(x, n_fft, hop_length, win_length, center, extra)
    nb = n_fft // 2 + 1
    dim = n_chroma if kind == "chroma" else 6
    if X.shape[0] == 0:
        return np.zeros((0, dim)), np.zeros((0, dim))
    W = filterbank32(sr, n_fft, n_chroma, tuning, ctroct, octwidth, base_c).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        S, dS = lm.power_bound(X, B, power)
        R = S @ W.T
    bad = ~np.isfinite(R).all(axis=1)
    S, dS = np.where(bad[:, None], 0.0, S), np.where(bad[:, None], 0.0, dS)
    R = S @ W.T
    if lm.is_pow2(n_fft):
        m = -(-nb // 64) + 6
    else:
        m = 4 + 6 + -(-nb // 256)
    dW = 2.0 * U * W + FLT_MIN
    dR = dS @ W.T + (S + dS) @ dW.T
    dR = dR + _gamma(m) * (R + dR)
    row, drow = normalize(R, dR, NORMS[chroma_norm])
    if kind == "tonnetz":
        u, du = normalize(row, drow, 1)
        P = np.abs(phi(n_chroma))
        row = u @ phi(n_chroma).T
        drow = du @ P.T + (U + _gamma(n_chroma)) * ((np.abs(u) + du) @ P.T)
    row[bad] = np.nan
    drow[bad] = 0.0
    return row, drow


def check(got, x, kind, sr, n_fft, hop_length, what="", **kw):
    """Asserts that got (the device's rows of one segment) is within the bound of the model on x, every value, and that exactly the
    model's non-finite frames are all NaN. Returns the worst |d| / bound."""
    want, tol = rows(x, kind, sr, n_fft, hop_length, **kw)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    if not want.size:
        return 0.0
    bad = np.isnan(want).all(axis=1)
    assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all(), (what, "non-finite frames", np.argwhere(bad)[:4])
    d = np.abs(got[~bad].astype(np.float64) - want[~bad])
    t = tol[~bad]
    ok = d <= t
    assert ok.all(), (what, kind, int((~ok).sum()), np.argwhere(~ok)[:4], float(np.max(d / np.maximum(t, 1e-300))))
    nz = t > 0
    return float((d[nz] / t[nz]).max()) if nz.any() else 0.0
