"""The float64 model of the pitch stage (include/vorbis_synth_hip.h, "pitch", steps 2 to 8), written out step by step. It is the
contract the device is compared against; tests/test_pitch_cpu.py compares it against a restatement in librosa's own words.

The difference function and its cumulative sum are taken in np.longdouble (64-bit mantissa here): every difference z[j] - z[j+tau]
of two float32 values is exact in float64, its square is formed and summed in longdouble, and one rounding to float64 follows, as
tests/trim_model.py does for its frame sums. The terms are non-negative, so the relative error of a sum is at most (terms) * 2^-64,
2^-11 of the device's float64 chain."""
import math
from fractions import Fraction

import numpy as np

TINY = 2.2250738585072014e-308  # numpy.finfo(float64).tiny
U = 2.0 ** -53


def num_frames(T, L, H, center=True):
    """Step 2: the frame count of "spectral features" step 2 with n_fft = L."""
    if T == 0:
        return 0
    tp = T + (2 * (L // 2) if center else 0)
    return 0 if tp < L else 1 + (tp - L) // H


def periods(sr, fmin, fmax, L):
    """Step 3 in double, as the host computes it: (p_min, p_max), or None with fewer than two lags."""
    W = L // 2
    lo = max(math.floor(float(sr) / float(fmax)), 1)
    hi = min(math.ceil(float(sr) / float(fmin)), L - W - 1)
    return (int(lo), int(hi)) if hi - lo + 1 >= 2 else None


def band(L, p_max):
    """The relative distance inside which two float64 evaluations of a comparison between two values of c (or between one and the
    threshold) may disagree. One evaluation of c[i] rounds: d, a chain of W = L // 2 fused multiply-adds of non-negative terms, at
    most W * 2^-53 relative; S, a sum of at most p_max such d in any order, at most p_max * 2^-53 more; S / tau, the addition of
    tiny and the division, 3 more: (W + p_max + 3) * 2^-53. A comparison has two sides, and the model and the device are two
    evaluations: twice that, with 2 W <= L."""
    return (L + 2 * p_max + 6) * U


def frames_of(y, L, H, center=True):
    """Step 2: the (F, L) float64 frames z of the mono signal y (float32 values), zeros outside [0, T)."""
    y = np.asarray(y, np.float64)
    T = y.shape[0]
    F = num_frames(T, L, H, center)
    if F == 0:
        return np.zeros((0, L), np.float64)
    pad = L // 2 if center else 0
    buf = np.zeros(max((F - 1) * H + L, pad + T), np.float64)
    buf[pad:pad + T] = y
    return np.lib.stride_tricks.sliding_window_view(buf, L)[::H][:F]


def difference(z, p_max):
    """Step 4 for one frame z (L,) float64 holding float32 values: d[tau - 1], tau = 1 .. p_max, as np.longdouble (p_max,)."""
    W = z.shape[0] // 2
    lag = np.lib.stride_tricks.sliding_window_view(z[2:], W)[:p_max]  # row tau - 1: z[1 + tau .. W + tau]
    d = np.empty(p_max, np.longdouble)
    step = max(1, (1 << 21) // max(W, 1))
    for a in range(0, p_max, step):
        diff = (z[1:W + 1][None, :] - lag[a:a + step]).astype(np.longdouble)  # exact in float64
        d[a:a + step] = (diff * diff).sum(axis=1)
    return d


def difference_fsum(z, tau):
    """One value of step 4 by math.fsum, which rounds the exact sum once: every square is taken exactly as a Fraction and handed
    over as two floats, hi + lo (a square of a float64 has at most 106 bits)."""
    W = len(z) // 2
    parts = []
    for j in range(1, W + 1):
        sq = Fraction(float(z[j]) - float(z[j + tau])) ** 2
        hi = float(sq)
        parts += [hi, float(sq - Fraction(hi))]
    return math.fsum(parts)


def exact_frame(z):
    """True for a frame whose samples are all multiples of 2^-12 of magnitude at most 1 (all zeros; a click of 0.5 in silence).
    Every square is then a multiple of 2^-24 below 2^2 and every sum of up to 2^24 of them is below 2^53 in units of 2^-24: d
    and S round nowhere, in any order, so two evaluations give the same bits of c and decide every comparison alike, ties included.
    The margin of such a frame is infinite, as that of a comparison of two exact zeros is."""
    q = z * 4096.0
    return bool((q == np.round(q)).all() and (np.abs(z) <= 1.0).all())


def cmnd(z, p_min, p_max):
    """Steps 4 and 5 for one frame: (c (n,) float64, d (p_max,) float64)."""
    d = difference(z, p_max)
    S = np.cumsum(d)  # longdouble, non-negative terms
    d64, S64 = d.astype(np.float64), S.astype(np.float64)
    tau = np.arange(p_min, p_max + 1, dtype=np.float64)
    return d64[p_min - 1:] / (S64[p_min - 1:] / tau + TINY), d64


def _gap(x, y):
    """|x - y| / max(|x|, |y|); two exact zeros count as decided (inf)."""
    m = np.maximum(np.abs(x), np.abs(y))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(m == 0.0, np.inf, np.abs(x - y) / np.where(m == 0.0, 1.0, m))


def pick(c, thr):
    """Steps 6 and 7 on one frame's c: dict(i, branch, a, b, shift, margin)."""
    n = c.shape[0]
    tr = np.zeros(n, bool)
    tr[1:-1] = (c[1:-1] < c[:-2]) & (c[1:-1] <= c[2:])
    tr[0] = c[0] < c[1]
    tr[-1] = c[-1] < c[-2]
    cand = np.flatnonzero(tr & (c < thr))
    t = np.full(n, thr)
    if cand.size:
        i, branch = int(cand[0]), "trough"
        k = i + 1  # every comparison that the indices up to i took part in
        gaps = [_gap(c[:k], t[:k]), _gap(c[1:k], c[:k - 1]) if k > 1 else np.array([np.inf]), _gap(c[:min(k, n - 1)], c[1:min(k, n - 1) + 1])]
    else:
        i, branch = int(np.argmin(c)), "minimum"
        others = np.delete(c, i)
        gaps = [_gap(np.full(n - 1, c[i]), others), _gap(c, t)]  # (and no c[i] may sit at the threshold: the branch itself)
    a = b = shift = 0.0
    if 0 < i < n - 1:
        a = (c[i + 1] + c[i - 1]) - 2.0 * c[i]
        b = (c[i + 1] - c[i - 1]) / 2.0
        gaps.append(_gap(np.array([abs(a)]), np.array([abs(b)])))
        if abs(b) < abs(a):
            shift = -b / a
    return dict(i=i, branch=branch, a=float(a), b=float(b), shift=float(shift), margin=float(min(g.min() for g in gaps)))


def f0_tolerance(c, r, L, p_min, p_max):
    """The relative bound on |f0_device - f0_model| before the float32 rounding, from band, |a| and the period. Each c the shift
    reads is off by at most band / 2 * c on either side (band covers both sides of a comparison). With e = band / 2:
    |da| <= e (c+ + c- + 2 c0) + 4 U (c+ + c- + 2 c0) (the additions of a themselves), |db| <= e (c+ + c-) / 2 + 2 U (c+ + c-);
    shift = -b / a: |dshift| <= (|db| + |shift| |da|) / (|a| - |da|) + 2 U |shift|; f0 = sr / (period + shift):
    |df0| / f0 <= |dshift| / (period + shift) + 3 U. Returns inf where |da| >= |a|."""
    i = r["i"]
    period = p_min + i + r["shift"]
    if not 0 < i < c.shape[0] - 1 or r["shift"] == 0.0 and r["a"] == 0.0:
        return 3 * U
    e = band(L, p_max) / 2
    s = c[i + 1] + c[i - 1]
    da = (e + 4 * U) * (s + 2 * c[i])
    db = (e / 2 + 2 * U) * s
    if da >= abs(r["a"]):
        return float("inf")
    dshift = (db + abs(r["shift"]) * da) / (abs(r["a"]) - da) + 2 * U * abs(r["shift"])
    return dshift / period + 3 * U


def yin(y, sr, fmin, fmax, L=2048, H=512, thr=0.1, center=True):
    """Steps 2 to 8 on the mono signal y (T,) float32: dict(f0 (F,) float64 before the rounding to float32, c (F,) float64: c[i*],
    lag (F,) int: p_min + i*, branch (F,), a, b, shift, margin (F,), tol (F,): f0_tolerance, band, p_min, p_max, d: a list of
    the frames' d arrays). A signal with a sample that is not finite is refused (step 9): refused=True and NaN rows."""
    y = np.asarray(y, np.float32)
    p_min, p_max = periods(sr, fmin, fmax, L)
    F = num_frames(y.shape[0], L, H, center)
    out = dict(f0=np.zeros(F), c=np.zeros(F), lag=np.zeros(F, np.int64), branch=[], a=np.zeros(F), b=np.zeros(F), shift=np.zeros(F),
               margin=np.full(F, np.inf), tol=np.zeros(F), band=band(L, p_max), p_min=p_min, p_max=p_max, d=[], cs=[], refused=False)
    if not np.isfinite(y).all():
        out["refused"] = True
        out["f0"][:] = np.nan
        out["c"][:] = np.nan
        return out
    for f, z in enumerate(frames_of(y, L, H, center)):
        c, d = cmnd(z, p_min, p_max)
        r = pick(c, thr)
        i = r["i"]
        out["f0"][f] = float(sr) / (float(p_min + i) + r["shift"])
        out["c"][f] = c[i]
        out["lag"][f] = p_min + i
        out["branch"].append(r["branch"])
        for k in ("a", "b", "shift", "margin"):
            out[k][f] = r[k]
        if exact_frame(z):
            out["margin"][f] = np.inf
        out["tol"][f] = f0_tolerance(c, r, L, p_min, p_max)
        out["d"].append(d)
        out["cs"].append(c)
    return out


def cmnd_fft(z, p_min, p_max):
    """Steps 4 and 5 for one frame in librosa's own words (librosa.core.pitch._cumulative_mean_normalized_difference, >= 0.10), in
    float64 and without its zeroing of values below 1e-6 (include/vorbis_synth_hip.h, "pitch", step 4)."""
    L = z.shape[0]
    W = L // 2
    a = np.fft.rfft(z, L)
    b = np.fft.rfft(z[W:0:-1], L)
    acf = np.fft.irfft(a * b, L)[W:]
    energy = np.cumsum(z ** 2)
    energy = energy[W:] - energy[:-W]
    yin_frames = energy[:1] + energy - 2 * acf
    num = yin_frames[p_min:p_max + 1]
    cumulative_mean = np.cumsum(yin_frames[1:p_max + 1]) / np.arange(1, p_max + 1)
    return num / (cumulative_mean[p_min - 1:p_max] + TINY)
