"""Float64 model and per-value error bound of the constant-Q rows (include/vorbis_synth_hip.h, "constant-Q"), written
from the header and not from the kernel. librosa is not among the test dependencies; parity with it is not claimed: the transform
is the direct time-domain sum that librosa.cqt / librosa.vqt approximate.

Model. frequencies / lengths / wavelet are steps 1 to 4 with the header's operations in the header's order: every operation is a
correctly rounded IEEE one except exp2, which is the C library's on both sides (_exp2 below: math.exp2, or libm's exp2 through
ctypes where Python has none; the host side calls the same function, so N_k is bit-equal), and cos / sin (numpy's may differ from
the C library's in the last place of a double, which a float32 pair sees only when the double sits within 2^-29 of a rounding
boundary). transform() is step 5 as a plain sum per (t, k) over the float64 downmix; rows() applies steps 6 to 10.

Bound (u = 2^-24), per (t, k). With A = sum_m |y[t hop + m]| |b_k[m]| over the support (the float64 pairs' moduli):
  table    each stored component is the float32 rounding of the model's double: |d re|, |d im| <= u |b|, so the pair moves by at
           most sqrt(2) u |b|; s_k is stored as float32: u more on the product.
  downmix  the device adds the C planes in float32 in ascending order and multiplies by float32(1 / C): C roundings for C > 1
           (C - 1 additions, the product), and the constant's own rounding: each sample moves by at most g(C + 1) mean_c |x_c|;
           pushed through the sum with A' = sum_m (mean_c |x_c|)[t hop + m] |b_k[m]| in place of A. One channel: nothing.
  chain    a lane's fma chain has at most ceil(chunk / 64) terms a chunk, the wave's butterfly adds 6 roundings, and the chunks'
           sums are added in ascending order: one more rounding per chunk the support touches, at most floor((L_k - 2) / chunk) + 2
           of them. m = ceil(chunk / 64) + 6 + chunks; each component's sum is off by at most g(m) A.
  output   one float32 product with s_k per component; magnitude: the squares, their fma, the root (power 1) round: 3 u on |C| in
           all, 4 u on |C|^2 (power 2) with the factor 2 of the square.
So per component dC = s_k (g(m + 2) + sqrt(2) u) A + s_k g(C + 1) A' (C > 1) + u |C_component|, and the modulus moves by at most
sqrt(2) of that. Chroma: the fold adds magnitudes (all >= 0) in ascending k, at most n_bins roundings: dR[c] = sum_k M dmag +
g(n_bins) (R + sum_k M dmag); the norm, the division and the tonnetz product propagate as tests/chroma_model.normalize does it.
No factor here is fitted to a case."""
import math

import numpy as np

from tests import chroma_model as cm

U = 2.0 ** -24
C1 = 32.70319566257483
HANN_BW = 1.50018310546875
MAX_L0 = 1 << 17
MAX_TABLE = 1 << 23
OUTPUTS = {"magnitude": 1, "complex": 2, "chroma": 3, "tonnetz": 4}


if hasattr(math, "exp2"):
    _exp2 = math.exp2
else:
    import ctypes
    import ctypes.util
    _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    _libm.exp2.argtypes, _libm.exp2.restype = [ctypes.c_double], ctypes.c_double
    _exp2 = _libm.exp2


def _g(m):
    return m * U / (1.0 - m * U)


def spec(n_bins=84, bins_per_octave=12, hop_length=512, fmin=None, tuning=0.0, filter_scale=1.0, gamma=0.0, norm=1, scale=True,
         output="magnitude", power=1, n_chroma=12, chroma_norm=np.inf, base_c=True):
    """The parameters as one dict (what every function here takes as sp)."""
    return dict(n_bins=n_bins, bins_per_octave=bins_per_octave, hop_length=hop_length, fmin=C1 if fmin is None else float(fmin),
                tuning=float(tuning), filter_scale=float(filter_scale), gamma=float(gamma), norm=norm, scale=scale, output=output,
                power=power, n_chroma=n_chroma, chroma_norm=chroma_norm, base_c=base_c)


def frequencies(sp):
    """f_k of step 1, a list of doubles: (fmin * exp2(tuning / bpo)) * exp2(k / bpo)."""
    bpo = float(sp["bins_per_octave"])
    f0 = sp["fmin"] * _exp2(sp["tuning"] / bpo)
    return [f0 * _exp2(float(k) / bpo) for k in range(sp["n_bins"])]


def quality(sp):
    """(alpha, Q) of step 2."""
    r = _exp2(1.0 / float(sp["bins_per_octave"]))
    alpha = (r * r - 1.0) / (r * r + 1.0)
    return alpha, sp["filter_scale"] / alpha


def lengths(sp, sr):
    """(N [n_bins] doubles, L [n_bins] ints, h [n_bins] ints = ceil(N / 2)) of steps 2 and 3."""
    alpha, Q = quality(sp)
    N = [Q * float(sr) / (f + sp["gamma"] / alpha) for f in frequencies(sp)]
    h = [int(math.ceil(n / 2.0)) for n in N]
    L = [hh + int(math.floor(n / 2.0)) for hh, n in zip(h, N)]
    return N, L, h


def rate_refused(sp, sr):
    """Step 10's test."""
    _, Q = quality(sp)
    return frequencies(sp)[-1] * (1.0 + 0.5 * HANN_BW / Q) > float(sr) / 2.0


def wavelet(sp, sr, k):
    """b_k [L_k] complex128 of step 4 (index j = m + ceil(N_k / 2)), and N_k."""
    N, L, h = lengths(sp, sr)
    f = frequencies(sp)[k]
    Lk = L[k]
    j = np.arange(Lk, dtype=np.float64)
    win = 0.5 - 0.5 * np.cos(2.0 * math.pi * j / float(Lk))
    if sp["norm"] == 1:
        n = float(np.cumsum(win)[-1])  # (added in ascending j, as the header has it)
    elif sp["norm"] == 2:
        n = math.sqrt(float(np.cumsum(win * win)[-1]))
    else:
        n = 1.0
    m = j - float(h[k])
    ph = 2.0 * math.pi * f * m / float(sr)
    return (win * np.cos(ph) / n) + 1j * (-(win * np.sin(ph)) / n), N[k]


def num_frames(sp, T):
    return 0 if T == 0 else 1 + T // sp["hop_length"]


def planes(x):
    x = np.asarray(x)
    return x[None, :] if x.ndim == 1 else x


def downmix(x):
    """(y float64 [T], a float64 [T] = mean_c |x_c|)."""
    x = planes(x).astype(np.float64)
    return x.mean(axis=0), np.abs(x).mean(axis=0)


def transform(y, sp, sr, absolute=False):
    """C [F][n_bins] complex128 of step 5, s_k applied. absolute=True: s_k sum_m y |b_k| instead (real; for y >= 0 the bound's A)."""
    y = np.asarray(y, np.float64)
    T, hop, nb = len(y), sp["hop_length"], sp["n_bins"]
    F = num_frames(sp, T)
    N, L, h = lengths(sp, sr)
    out = np.zeros((F, nb), np.float64 if absolute else np.complex128)
    for k in range(nb):
        b, Nk = wavelet(sp, sr, k)
        if absolute:
            b = np.abs(b)
        s = math.sqrt(Nk) if sp["scale"] else Nk
        for t in range(F):
            lo = t * hop - h[k]
            a, e = max(lo, 0), min(lo + L[k], T)
            if e > a:
                out[t, k] = s * np.dot(y[a:e], b[a - lo:e - lo])
    return out


def chunks_touched(Lk, chunk):
    return (Lk - 2) // chunk + 2 if Lk >= 2 else 1


def cq_classes(sp):
    """The chroma class of every bin (step 7), from the closed expression of the header."""
    bpo, nc = sp["bins_per_octave"], sp["n_chroma"]
    nm = bpo // nc
    midi0 = math.fmod(12.0 * (math.log2(sp["fmin"]) - math.log2(440.0)) + 69.0, 12.0)
    if midi0 < 0.0:
        midi0 += 12.0
    roll = midi0 if sp["base_c"] else midi0 - 9.0
    roll = int(np.round(roll * (nc / 12.0)))
    return [((((k % bpo) + nm // 2) % bpo) // nm + roll) % nc for k in range(sp["n_bins"])]


def rows(x, sp, sr, chunk):
    """(want [F][dim] float64 (complex output: re, im interleaved), bound [F][dim]) of planar x [C][T] or mono [T] at rate sr. A
    refused segment (step 9 or 10) is all NaN with bound 0."""
    X = planes(x)
    Cn, T = X.shape
    nb, out = sp["n_bins"], sp["output"]
    F = num_frames(sp, T)
    dim = {"magnitude": nb, "complex": 2 * nb, "chroma": sp["n_chroma"], "tonnetz": 6}[out]
    if F == 0:
        return np.zeros((0, dim)), np.zeros((0, dim))
    if rate_refused(sp, sr) or not np.isfinite(X).all():
        return np.full((F, dim), np.nan), np.zeros((F, dim))
    y, a = downmix(X)
    Cx = transform(y, sp, sr)
    A = transform(np.abs(y), sp, sr, absolute=True)
    N, L, _ = lengths(sp, sr)
    m = np.array([-(-chunk // 64) + 6 + chunks_touched(l, chunk) for l in L], np.float64)
    comp = (_g(m + 2.0) + math.sqrt(2.0) * U)[None, :] * A
    if Cn > 1:
        comp = comp + _g(Cn + 1.0) * transform(a, sp, sr, absolute=True)
    if out == "complex":
        want = np.empty((F, dim))
        want[:, 0::2], want[:, 1::2] = Cx.real, Cx.imag
        tol = np.empty((F, dim))
        tol[:, 0::2] = comp + U * np.abs(Cx.real)
        tol[:, 1::2] = comp + U * np.abs(Cx.imag)
        return want, tol
    mag = np.abs(Cx)
    dmag = math.sqrt(2.0) * (comp + U * mag) + 3.0 * U * mag
    if out == "magnitude":
        if sp["power"] == 1:
            return mag, dmag
        return mag * mag, (2.0 * mag + dmag) * dmag + 4.0 * U * mag * mag
    cls = cq_classes(sp)
    M = np.zeros((sp["n_chroma"], nb))
    M[cls, np.arange(nb)] = 1.0
    R = mag @ M.T
    dR = dmag @ M.T
    dR = dR + _g(nb) * (R + dR)
    row, drow = cm.normalize(R, dR, cm.NORMS[sp["chroma_norm"]])
    if out == "tonnetz":
        u, du = cm.normalize(row, drow, 1)
        P = np.abs(cm.phi(sp["n_chroma"]))
        row = u @ cm.phi(sp["n_chroma"]).T
        drow = du @ P.T + (U + _g(sp["n_chroma"])) * ((np.abs(u) + du) @ P.T)
    return row, drow


def bound(x, sp, sr, chunk):
    return rows(x, sp, sr, chunk)[1]


def check(got, x, sp, sr, chunk, what=""):
    """Asserts |device - model| <= bound for every value of one segment's rows, nothing excluded, and that a refused segment is all
    NaN. Returns the worst |d| / bound."""
    want, tol = rows(x, sp, sr, chunk)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    if not want.size:
        return 0.0
    if np.isnan(want).all():
        assert np.isnan(got).all(), (what, "a refused segment's rows must be NaN")
        return 0.0
    assert np.isfinite(got).all(), (what, "non-finite values", np.argwhere(~np.isfinite(got))[:4])
    d = np.abs(got.astype(np.float64) - want)
    ok = d <= tol
    assert ok.all(), (what, int((~ok).sum()), np.argwhere(~ok)[:4], float(np.max(d / np.maximum(tol, 1e-300))))
    nz = tol > 0
    return float((d[nz] / tol[nz]).max()) if nz.any() else 0.0
