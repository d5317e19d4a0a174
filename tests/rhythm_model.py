"""Float64 model of the rhythm stages (include/vorbis_synth_hip.h, "rhythm"): onset strength, onset frames, tempogram, its mean and
the tempo, with the error bounds the GPU tests gate on. numpy only; tests/test_rhythm_cpu.py checks it against restatements in
numpy's and scipy's own words.

Bounds, u = 2^-24 (float32), e = 2^-53 (float64):
  onset strength   the model adds in the device's documented order, so the float64 sums agree unless an addition is not correctly
                   rounded; the gate still allows what any order may cost: |d| <= u |v| + 12 e |v| + 2^-126 (one rounding to float32,
                   a subtraction per term, nine additions down a term's path, a division; a flushed denormal).
  tempogram        ac[l] is an fma chain of n = W - l terms on the device and numpy's dot here: each is within n e A[l] of the exact
                   sum, A[l] = sum |y[n] y[n + l]|, so they differ by at most 2 n e A[l]. Through the norm (v = ac / mx) and the
                   rounding: see tempogram().
  mean             the float32 rows are added in float64: F' terms, (F' + 1) e mean|row| on top of the mean of the rows' bounds.
  comparisons      peak test (b) and the tempo arg-max are decisions: band_b() and tempo()'s band say how far two float64
                   evaluations may disagree, and the CPU tests assert every input decides by more.
"""
from fractions import Fraction

import numpy as np

U32 = 2.0 ** -24
E64 = 2.0 ** -53
FLT_MIN = float(np.finfo(np.float32).tiny)
TINY = 2.0 ** -126
MAX_BLOCKS = 128


def reflect(i, n):
    """numpy.pad(mode="symmetric") of an index, as often as needed."""
    m = i % (2 * n)
    return 2 * n - 1 - m if m >= n else m


# ---- A. onset strength ----------------------------------------------------------------------------------------------------------
def ref_rows(S, m):
    """Step A.1: maximum over [j - m/2, j - m/2 + m) with symmetric reflection; a window that holds a NaN gives NaN."""
    S = np.asarray(S, np.float32)
    if m == 1:
        return S.copy()
    D = S.shape[1]
    idx = np.array([[reflect(j - m // 2 + k, D) for k in range(m)] for j in range(D)])  # (D, m)
    win = S[:, idx]  # (F, D, m)
    with np.errstate(invalid="ignore"):
        out = win.max(axis=2)  # numpy's max hands a NaN on
    return out.astype(np.float32)


def onset_p(n_fft, hop, center):
    return n_fft // (2 * hop) if center else 0


def _ordered_sum(terms):
    """Step A.3 on (F, D) float64 terms: 64 partials of the bins i, i + 64, .. then the xor rounds 32 .. 1."""
    F, D = terms.shape
    part = np.zeros((F, 64))
    for k in range(0, D, 64):
        blk = terms[:, k:k + 64]
        part[:, :blk.shape[1]] = part[:, :blk.shape[1]] + blk
    lanes = np.arange(64)
    o = 32
    while o >= 1:
        part = part + part[:, lanes ^ o]
        o >>= 1
    return part[:, 0]


def onset_strength64(S, lag=1, max_size=1, n_fft=2048, hop=512, center=True):
    """env as float64 before its one rounding, F entries."""
    S = np.asarray(S, np.float32)
    F, D = S.shape
    p = onset_p(n_fft, hop, center)
    env = np.zeros(F)
    n = F - p - lag  # entries f = p + lag .. F - 1
    if n <= 0:
        return env
    R = ref_rows(S, max_size).astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = S[lag:lag + n].astype(np.float64) - R[:n]
        t = np.maximum(0.0, d)  # numpy.maximum: a NaN stays
        t = np.where(t == 0.0, 0.0, t)  # (-0 cannot arise from max(0, .), kept for clarity)
        env[p + lag:] = _ordered_sum(t) / D
    return env


def onset_strength(S, **kw):
    with np.errstate(over="ignore"):
        return onset_strength64(S, **kw).astype(np.float32)


def onset_gate(got, S, **kw):
    """Asserts the gate on one segment; returns the worst |d| / tolerance."""
    v = onset_strength64(S, **kw)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == v.shape, (got.dtype, got.shape, v.shape)
    nan = np.isnan(v)
    assert np.array_equal(np.isnan(got), nan)
    inf = np.isinf(v)
    assert np.array_equal(got[inf].astype(np.float64), v[inf])
    fin = ~nan & ~inf
    big = np.abs(v) > float(np.finfo(np.float32).max)  # rounds to Inf
    assert np.all(np.isinf(got[fin & big]))
    fin &= ~big
    tol = (U32 + 12 * E64) * np.abs(v[fin]) + TINY
    d = np.abs(got[fin].astype(np.float64) - v[fin])
    assert np.all(d <= tol), float((d / tol).max())
    return float((d / tol).max()) if d.size else 0.0


# ---- B. onset frames ------------------------------------------------------------------------------------------------------------
PEAK_TIMES = dict(pre_max=0.03, post_max=0.0, pre_avg=0.10, post_avg=0.10, wait=0.03)


def peak_windows(rate, hop, pre_max=0.03, post_max=0.0, pre_avg=0.10, post_avg=0.10, wait=0.03):
    """Step B.1: (pre_max, post_max, pre_avg, post_avg, wait) in frames."""
    w = lambda t: int(np.floor((float(t) * float(rate)) / float(hop)))  # noqa: E731
    return w(pre_max), w(post_max) + 1, w(pre_avg), w(post_avg) + 1, w(wait)


def _normalised(x, normalize):
    x = np.asarray(x, np.float32)
    if not normalize or not len(x):
        return x.astype(np.float64)
    mn, mx = float(x.min()), float(x.max())
    return (x.astype(np.float64) - mn) / ((mx - mn) + FLT_MIN)


def peak_pick(x, windows, delta=0.07, normalize=True):
    """Steps B.2 to B.5 on a float32 envelope: (int64 frames, refused). A literal loop."""
    x = np.asarray(x, np.float32)
    F = len(x)
    if not np.all(np.isfinite(x)):
        return np.zeros(0, np.int64), True
    pre_max, post_max, pre_avg, post_avg, wait = windows
    u = _normalised(x, normalize)
    out, last = [], None
    for n in range(F):
        if x[n] < x[max(0, n - pre_max):min(F, n + post_max)].max():
            continue
        b0, b1 = max(0, n - pre_avg), min(F, n + post_avg)
        s = 0.0
        for k in range(b0, b1):
            s += u[k]
        if not u[n] >= s / (b1 - b0) + delta:
            continue
        if last is None or n - last > wait:
            out.append(n)
            last = n
    return np.array(out, np.int64), False


def band_b(x, windows, delta=0.07, normalize=True):
    """For every frame that passes test (a): how far comparison (b) is from the band inside which two float64 evaluations can
    disagree. Returns the smallest |exact u[n] - mean - delta| / band over those frames (Inf when there is none); a frame whose window
    is all zeros with delta = 0 is exact in any evaluation and is left out. band = e (4 |u[n]| + (count + 6) mean|u| + 2 |delta|):
    two roundings in a u (four with the denominator's), count - 1 additions, the division and the addition of delta."""
    x = np.asarray(x, np.float32)
    F = len(x)
    pre_max, post_max, pre_avg, post_avg, _ = windows
    X = [Fraction(float(v)) for v in x]
    if normalize:
        mn, mx = min(X), max(X)
        den = mx - mn + Fraction(FLT_MIN)
        U = [(v - mn) / den for v in X]
    else:
        U = X
    worst = np.inf
    for n in range(F):
        if x[n] < x[max(0, n - pre_max):min(F, n + post_max)].max():
            continue
        b0, b1 = max(0, n - pre_avg), min(F, n + post_avg)
        win = U[b0:b1]
        if delta == 0 and all(v == 0 for v in win):
            continue
        mean = sum(win) / (b1 - b0)
        exact = abs(U[n] - mean - Fraction(float(delta)))
        band = E64 * (4 * abs(U[n]) + (b1 - b0 + 6) * sum(abs(v) for v in win) / (b1 - b0) + 2 * abs(Fraction(float(delta))))
        worst = min(worst, float(exact / band) if band else np.inf)
    return worst


# ---- C. tempogram ---------------------------------------------------------------------------------------------------------------
def hann(W):
    """scipy.signal.get_window("hann", W, fftbins=True) rounded to float32."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W) / W)).astype(np.float32)


def pad_env(e, W):
    """Step C.1: numpy.pad(e, W // 2, mode="linear_ramp", end_values=0) on float32."""
    e = np.asarray(e, np.float32)
    w = W // 2
    if not len(e):
        return e
    with np.errstate(invalid="ignore", over="ignore"):
        left = (np.arange(w, dtype=np.float64) * (float(e[0]) / w)).astype(np.float32)
        right = (np.arange(w - 1, -1, -1, dtype=np.float64) * (float(e[-1]) / w)).astype(np.float32)
    return np.concatenate([left, e, right])


def tg_rows(F, W, center):
    return F if center else max(0, F - W + 1)


def tg_tile(W):
    """Rows per tile (vsyn_tempogram_tile): a multiple of 4, at most 32, 8 (2 FT + 1) W bytes within 79 KiB; 4 always."""
    ft = 32
    while ft > 4 and 8 * (2 * ft + 1) * W > 79 * 1024:
        ft -= 4
    return ft


def tempogram(e, W=384, center=True, norm=True, only=None):
    """(rows float32 (F', W), bound float64 (F', W)): the rows and how far a correct device value may lie from them; only: a list of
    frames, and the two arrays hold those frames alone (a long segment at a large W costs W^2 a frame here).
    With v = ac / mx: |dv| <= dac / mx + |v| dmx / mx + e |v| (dac, dmx: 2 n e A of the lag and of the largest lag bound), and the
    gate is dv (1 + u) + u |v| + 2^-126. A row with a non-finite value has bound NaN: compare its pattern instead."""
    e = np.asarray(e, np.float32)
    F = len(e)
    Fp = tg_rows(F, W, center)
    frames = list(range(Fp)) if only is None else [int(f) for f in only]
    rows = np.zeros((len(frames), W), np.float32)
    bound = np.zeros((len(frames), W))
    if not frames:
        return rows, bound
    ep = pad_env(e, W).astype(np.float64) if center else e.astype(np.float64)
    win = hann(W).astype(np.float64)
    n_terms = (W - np.arange(W)).astype(np.float64)
    for i, f in enumerate(frames):
        with np.errstate(invalid="ignore", over="ignore"):
            y = win * ep[f:f + W]
            if not np.all(np.isfinite(y)):
                ac = np.array([np.sum(y[:W - l] * y[l:]) for l in range(W)])
            else:
                ac = np.correlate(y, y, "full")[W - 1:]
            a = np.abs(y)
            dac = 2.0 * n_terms * E64 * (np.correlate(a, a, "full")[W - 1:] if np.all(np.isfinite(y)) else np.nan)
            v, dv = ac, dac
            if norm:
                mx = np.abs(ac).max()  # NaN when a NaN is among them
                if not mx <= FLT_MIN:
                    v = ac / mx
                    dv = dac / mx + np.abs(v) * dac.max() / mx + E64 * np.abs(v)
            rows[i] = v.astype(np.float32)
            bound[i] = dv * (1 + U32) + U32 * np.abs(v) + TINY
    return rows, bound


def tg_norm_margin(e, W=384, center=True):
    """The smallest max |ac| over the rows that is not 0: the norm's threshold test (mx <= FLT_MIN) is decided when this is far from
    FLT_MIN and the rest are exact zeros."""
    rows, _ = tempogram(e, W, center, norm=False)
    mx = np.abs(rows.astype(np.float64)).max(axis=1) if len(rows) else np.zeros(0)
    return float(mx[mx > 0].min()) if np.any(mx > 0) else np.inf


def tg_gate(got, e, W=384, center=True, norm=True, only=None):
    """Asserts the per-value gate on one segment's rows (only: on those frames of it); returns the worst |d| / bound over the finite
    rows."""
    rows, bound = tempogram(e, W, center, norm, only)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == (tg_rows(len(e), W, center), W), got.shape
    if only is not None:
        got = got[[int(f) for f in only]]
    bad = ~np.isfinite(bound).all(axis=1) | ~np.isfinite(rows).all(axis=1)
    assert np.array_equal(np.isnan(got[bad]), np.isnan(rows[bad]))
    ok = ~bad
    d = np.abs(got[ok].astype(np.float64) - rows[ok].astype(np.float64))
    # the model's own float32 rounding is one of the u |v| in the bound's budget: the device value lies within bound of the float64 v,
    # and rows is v rounded, so allow that rounding once more
    tol = bound[ok] + U32 * np.abs(rows[ok].astype(np.float64))
    assert np.all(d <= tol), float((d / tol).max())
    return float((d / tol).max()) if d.size else 0.0


def tg_blocks(Fp, W):
    """Step C.4's blocked order: (rows per block, blocks)."""
    ft = tg_tile(W)
    tiles = -(-Fp // ft)
    tpb = max(1, -(-tiles // MAX_BLOCKS))
    return ft * tpb, -(-tiles // tpb)


def tg_mean(rows):
    """Step C.4 on float32 rows (F', W), in the documented blocked order: g float64 (W,). F' = 0: NaN."""
    rows = np.asarray(rows, np.float32)
    Fp, W = rows.shape
    if Fp == 0:
        return np.full(W, np.nan)
    per, nb = tg_blocks(Fp, W)
    g = np.zeros(W)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(nb):
            s = np.zeros(W)
            for r in rows[b * per:(b + 1) * per].astype(np.float64):
                s = s + r
            g = g + s
        return g / Fp


def tg_mean_bound(rows, bound):
    """How far a device mean may lie from tg_mean(model rows): the mean of the rows' bounds plus (F' + 1) e mean|row|."""
    Fp = len(rows)
    return bound.mean(axis=0) + (Fp + 1) * E64 * np.abs(rows.astype(np.float64)).mean(axis=0)


# ---- tempo ----------------------------------------------------------------------------------------------------------------------
def tempo(g, rate, hop, start_bpm=120.0, std_bpm=1.0, max_tempo=320.0):
    """Step C.5: (bpm, lag, margin, band). margin: the winning score minus the best other one; band: how far two float64 evaluations
    of that difference can disagree, 8 e (|log1p| + |prior|) of either score (log1p and log2 within an ulp or two, the square,
    the product, the sum). max_tempo None or 0: no cap."""
    g = np.asarray(g, np.float64)
    W = len(g)
    assert np.all(np.isfinite(g)) and np.all(g >= -1e-6)
    with np.errstate(divide="ignore"):
        bpm = 60.0 * float(rate) / (float(hop) * np.arange(W, dtype=np.float64))
    bpm[0] = np.inf
    with np.errstate(invalid="ignore"):
        prior = -0.5 * ((np.log2(bpm) - np.log2(start_bpm)) / std_bpm) ** 2
    if max_tempo:
        prior[:int(np.argmax(bpm < max_tempo))] = -np.inf
    a = np.log1p(1e6 * g)
    score = a + prior
    lag = int(np.argmax(score))
    rest = np.delete(score, lag)
    margin = float(score[lag] - rest.max()) if len(rest) else np.inf
    fin = np.isfinite(score)
    band = 16 * E64 * float((np.abs(a[fin]) + np.abs(prior[fin])).max()) if fin.any() else 0.0
    return float(bpm[lag]), lag, margin, band


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def rows(F, D, seed, kind="db"):
    """Synthetic spectral rows: dB-like values in [-80, 0] with structure along time, or non-negative power rows."""
    r = np.random.default_rng(seed)
    x = r.standard_normal((F, D)) * 6.0 + 10.0 * np.sin(np.arange(F)[:, None] * 0.37 + np.arange(D)[None, :] * 0.11) - 40.0
    if kind == "power":
        x = 10.0 ** (x / 10.0)
    return x.astype(np.float32)


def envelope(F, seed, negative=False):
    r = np.random.default_rng(seed)
    x = r.random(F) ** 3 * 4.0
    if negative:
        x = x - 1.0
    return x.astype(np.float32)


def click_train(F=600, period=20, first=5, noise=0.01, seed=3):
    r = np.random.default_rng(seed)
    x = noise * r.random(F)
    x[first::period] = 1.0
    return x.astype(np.float32)
