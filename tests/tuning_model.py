"""Model of the tuning estimation (include/vorbis_synth_hip.h, "tuning estimation"): piptrack's peaks and the tuning
taken from them. librosa is not a test dependency; the contract is the header's arithmetic, restated here.

Three layers:

  piptrack(S, ...)       steps 3 to 5 on a float32 spectrogram S [F][NB], operation for operation in float32 (the pitch through
                         double, as the header says): on the device's own S it reproduces the device bit for bit. piptrack_loop is
                         the same written as a plain loop over frames and bins, which the CPU tests hold against it.
  pitch_tuning(p, m, ..) steps 6 to 8 in float64 on pitch / mag arrays (float32): the median by numpy.median on float32, the histogram
                         by searchsorted on the header's edges, the first arg-max. It also names the bins that an entry within
                         1e-9 of an edge could move the answer to (the device's double log2 may differ from numpy's by an ulp).
  decisions(S, dS, ...)  the decision bands for a device S that is only known to lie in [S - dS, S + dS] (tests/spectral_lin_model.py:
                         stft and power_bound), and the bounds on pitch and mag at the decided peaks.

Decision bands. u = 2^-24, S the float64 model, dS its bound, both [F][NB]; everything per frame.
  ref = threshold32 * max_k S_dev[k] lies in [t (max_k (S - dS)) (1 - u), t (max_k (S + dS)) (1 + u)] = [ref_lo, ref_hi]: the maximum
    of values within their intervals lies between the maxima of the ends, and the product rounds once.
  Bin k is ABOVE (Z_dev[k] = S_dev[k] > 0) when S - dS > ref_hi, BELOW (Z_dev[k] = 0) when S + dS < ref_lo, else open.
  Z_dev[k] > Z_dev[j] for a neighbour j holds for sure when k is ABOVE and (j is BELOW, or S[k] - dS[k] > S[j] + dS[j]: Z_dev[j] is
    0 or S_dev[j], and S_dev[k] exceeds both). It fails for sure when k is BELOW, or when j is ABOVE and S[k] + dS[k] < S[j] - dS[j].
    The test >= against the right neighbour is decided by the same strict inequalities (equality is never decided).
  A bin is a decided peak when it is inside [k_lo, k_hi) and both neighbour tests hold for sure; a decided non-peak when it is outside
    the band or one test fails for sure; undecided otherwise. At the edges the replicated neighbour is the bin itself: bin 0 is a
    decided non-peak, bin NB - 1 needs the left test alone.
  At a decided peak with 1 <= k <= NB - 2, a = (S[k+1] - S[k-1]) / 2 and b = 2 S[k] - S[k+1] - S[k-1] of the model, and the device's
    a_dev = a +- da,  da = (dS[k+1] + dS[k-1]) / 2 + 2 u |a|          (one rounded difference; the halving is exact)
    b_dev = b +- db,  db = 2 dS[k] + dS[k+1] + dS[k-1] + 2 u (2 S[k] + S[k+1] + S[k-1])   (two rounded differences of such terms)
  The peak counts as decided only if |b| - db > FLT_MIN: then b_dev is neither replaced nor of the other sign, and
    s_dev = a_dev / b_dev (1 + e), |e| <= u:   |s_dev - s| <= ds = (da + |s| db) / (|b| - db) + 2 u |s|
    pitch = float32((k + s_dev) sr / n_fft):   |pitch_dev - pitch| <= ds sr / n_fft + u (|pitch| + ds sr / n_fft)
    mag = S_dev[k] + (a_dev / 2) s_dev:        t = a s / 2, dt = (|a| ds + |s| da + da ds) / 2 + 2 u |t|,
                                               |mag_dev - mag| <= dS[k] + dt + u (|mag| + dS[k] + dt)
  At k = NB - 1, s = 0 exactly: pitch is the bin's frequency rounded once and mag = S_dev[k] within dS[k].
"""
import numpy as np

U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
DEFAULTS = dict(fmin=150.0, fmax=4000.0, threshold=0.1, resolution=0.01, bins_per_octave=12)


def bins(sr, n_fft, fmin=150.0, fmax=4000.0):
    """[k_lo, k_hi) of step 2: the bins with fmin' <= k sr / n_fft < fmax'; (0, 0) when there is none."""
    lo, hi = max(float(fmin), 0.0), min(float(fmax), sr / 2.0)
    ks = [k for k in range(n_fft // 2 + 1) if lo <= k * sr / n_fft < hi]
    return (ks[0], ks[-1] + 1) if ks else (0, 0)


def piptrack(S, sr, n_fft, fmin=150.0, fmax=4000.0, threshold=0.1):
    """(pitch, mag) float32 [F][NB] of steps 3 to 5 on S float32 [F][NB], vectorised."""
    S = np.asarray(S)
    assert S.dtype == np.float32 and S.ndim == 2 and S.shape[1] == n_fft // 2 + 1
    F, nb = S.shape
    k_lo, k_hi = bins(sr, n_fft, fmin, fmax)
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(S).all(axis=1)
        Sf = np.where(bad[:, None], np.float32(0), S)
        ref = np.float32(threshold) * Sf.max(axis=1, keepdims=True, initial=np.float32(0))
        Z = np.where(Sf > ref, Sf, np.float32(0))
        Zp = np.pad(Z, ((0, 0), (1, 1)), mode="edge")
        k = np.arange(nb)
        peak = (Z > Zp[:, :-2]) & (Z >= Zp[:, 2:]) & ((k >= k_lo) & (k < k_hi))[None, :]
        Sp = np.pad(Sf, ((0, 0), (1, 1)), mode="edge")
        a = np.float32(0.5) * (Sp[:, 2:] - Sp[:, :-2])
        b = (np.float32(2) * Sf - Sp[:, 2:]) - Sp[:, :-2]
        b = np.where(np.abs(b) < np.float32(FLT_MIN), b + np.float32(1), b)
        s = a / b
        edge = (k == 0) | (k == nb - 1)
        a = np.where(edge[None, :], np.float32(0), a).astype(np.float32)
        s = np.where(edge[None, :], np.float32(0), s).astype(np.float32)
        pitch = ((k[None, :].astype(np.float64) + s.astype(np.float64)) * (float(sr) / n_fft)).astype(np.float32)
        mag = (Sf + (np.float32(0.5) * a) * s).astype(np.float32)
    pitch = np.where(peak, pitch, np.float32(0)).astype(np.float32)
    mag = np.where(peak, mag, np.float32(0)).astype(np.float32)
    pitch[bad] = np.nan
    mag[bad] = np.nan
    return pitch, mag


def piptrack_loop(S, sr, n_fft, fmin=150.0, fmax=4000.0, threshold=0.1):
    """piptrack as a plain loop over frames and bins, scalar float32 arithmetic."""
    S = np.asarray(S, np.float32)
    F, nb = S.shape
    f32 = np.float32
    k_lo, k_hi = bins(sr, n_fft, fmin, fmax)
    pitch, mag = np.zeros((F, nb), f32), np.zeros((F, nb), f32)
    for f in range(F):
        row = S[f]
        if not all(np.isfinite(v) for v in row):
            pitch[f], mag[f] = np.nan, np.nan
            continue
        mx = f32(0)
        for v in row:
            mx = v if v > mx else mx
        ref = f32(f32(threshold) * mx)
        z = [v if v > ref else f32(0) for v in row]
        for k in range(nb):
            zm, zp = z[max(k - 1, 0)], z[min(k + 1, nb - 1)]
            if not (k_lo <= k < k_hi and z[k] > zm and z[k] >= zp):
                continue
            a = s = f32(0)
            if 1 <= k <= nb - 2:
                a = f32(f32(0.5) * f32(row[k + 1] - row[k - 1]))
                b = f32(f32(f32(2) * row[k] - row[k + 1]) - row[k - 1])
                if abs(b) < f32(FLT_MIN):
                    b = f32(b + f32(1))
                s = f32(a / b)
            pitch[f, k] = f32((float(k) + float(s)) * (float(sr) / n_fft))
            mag[f, k] = f32(row[k] + f32(f32(f32(0.5) * a) * s))
    return pitch, mag


def edges(resolution):
    nbin = int(np.ceil(1.0 / resolution))
    return -0.5 + np.arange(nbin + 1, dtype=np.float64) * (1.0 / nbin)


def residuals(pitch, bins_per_octave=12):
    r = np.fmod(bins_per_octave * np.log2(np.asarray(pitch, np.float32).astype(np.float64) / 27.5), 1.0)
    return np.where(r >= 0.5, r - 1.0, r)


def pitch_tuning(pitch, mag=None, resolution=0.01, bins_per_octave=12):
    """Steps 6 to 8: dict(tuning, n, selected, admitted). pitch / mag: float32 arrays of any shape (NaN entries are not > 0 and take
    no part); mag None selects every entry with pitch > 0. admitted: the tunings that entries within 1e-9 of an edge could turn the
    answer into, tuning itself included; more than one element only when such an entry's bins compete for the arg-max."""
    p = np.asarray(pitch, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        keep = p > 0
    p = p[keep]
    n = int(p.size)
    if n == 0:
        return dict(tuning=0.0, n=0, selected=0, admitted=[0.0])
    if mag is not None:
        m = np.asarray(mag, np.float32).reshape(-1)[keep]
        thr = np.median(m)
        assert thr.dtype == np.float32
        sel = m >= thr
        p = p[sel]
    e = edges(resolution)
    nbin = e.size - 1
    r = residuals(p, bins_per_octave)
    idx = np.searchsorted(e, r, side="right") - 1
    ok = (idx >= 0) & (idx < nbin)
    counts = np.bincount(idx[ok], minlength=nbin)
    best = int(np.argmax(counts))
    near_lo = ok & (np.abs(r - e[np.clip(idx, 0, nbin - 1)]) < 1e-9)
    near_hi = ok & (np.abs(r - e[np.clip(idx + 1, 0, nbin)]) < 1e-9)
    moves = int(near_lo.sum() + near_hi.sum())
    admitted = [float(e[best])]
    if moves:
        touched = set(idx[near_lo | near_hi].tolist()) | set((idx[near_lo] - 1).tolist()) | set((idx[near_hi] + 1).tolist())
        for b in sorted(t for t in touched | {best} if 0 <= t < nbin):
            if counts[b] + moves >= counts[best] - moves and float(e[b]) not in admitted:
                admitted.append(float(e[b]))
        if len(admitted) > 1:  # the winner may lose entries: every bin that then reaches it competes
            for b in np.nonzero(counts + moves >= counts[best] - moves)[0]:
                if float(e[b]) not in admitted:
                    admitted.append(float(e[b]))
    return dict(tuning=float(e[best]), n=n, selected=int(p.size), admitted=admitted)


def decisions(S, dS, sr, n_fft, fmin=150.0, fmax=4000.0, threshold=0.1):
    """The decision bands of the module docstring on the float64 model S with bound dS, both [F][NB]: dict(peak, nonpeak (decided, bool
    [F][NB]; neither: undecided), pitch, dpitch, mag, dmag (float64, valid at decided peaks))."""
    S, dS = np.asarray(S, np.float64), np.asarray(dS, np.float64)
    F, nb = S.shape
    k_lo, k_hi = bins(sr, n_fft, fmin, fmax)
    t = float(np.float32(threshold))
    lo, hi = S - dS, S + dS
    ref_lo = t * lo.max(axis=1, keepdims=True) * (1.0 - U)
    ref_hi = t * hi.max(axis=1, keepdims=True) * (1.0 + U)
    above, below = lo > ref_hi, hi < ref_lo
    k = np.arange(nb)
    inband = ((k >= k_lo) & (k < k_hi))[None, :]

    def neighbour(shift):  # (holds for sure, fails for sure) of Z[k] > Z[k + shift], replicated edges
        j = np.clip(k + shift, 0, nb - 1)
        own = (j == k)[None, :]
        sure = above & (below[:, j] | (lo > hi[:, j])) & ~own
        fails = below | (above[:, j] & (hi < lo[:, j]))
        return sure, fails, own

    ls, lf, lown = neighbour(-1)
    rs, rf, rown = neighbour(+1)
    ls, lf = ls & ~lown, lf | lown           # Z[0] > Z[0] never holds
    rs = np.where(rown, above, rs)            # Z[NB-1] >= Z[NB-1] holds; the bin must still be ABOVE (a zero is no peak: Z > Z[k-1] >= 0)
    rf = np.where(rown, below, rf)
    peak = inband & ls & rs
    nonpeak = ~inband | lf | rf
    Sp, dSp = np.pad(S, ((0, 0), (1, 1)), mode="edge"), np.pad(dS, ((0, 0), (1, 1)), mode="edge")
    a = 0.5 * (Sp[:, 2:] - Sp[:, :-2])
    b = 2.0 * S - Sp[:, 2:] - Sp[:, :-2]
    da = 0.5 * (dSp[:, 2:] + dSp[:, :-2]) + 2.0 * U * np.abs(a)
    db = 2.0 * dS + dSp[:, 2:] + dSp[:, :-2] + 2.0 * U * (2.0 * S + Sp[:, 2:] + Sp[:, :-2])
    inner = ((k >= 1) & (k <= nb - 2))[None, :]
    safe = (np.abs(b) - db) > FLT_MIN
    peak = peak & (safe | ~inner)
    with np.errstate(all="ignore"):
        s = np.where(inner & safe, a / np.where(safe, b, 1.0), 0.0)
        ds = np.where(inner & safe, (da + np.abs(s) * db) / np.where(safe, np.abs(b) - db, 1.0) + 2.0 * U * np.abs(s), 0.0)
    a = np.where(inner, a, 0.0)
    da = np.where(inner, da, 0.0)
    hz = float(sr) / n_fft
    pitch = (k[None, :] + s) * hz
    dpitch = ds * hz + U * (np.abs(pitch) + ds * hz)
    tt = 0.5 * a * s
    dt = 0.5 * (np.abs(a) * ds + np.abs(s) * da + da * ds) + 2.0 * U * np.abs(tt)
    mag = S + tt
    dmag = dS + dt + U * (np.abs(mag) + dS + dt)
    return dict(peak=peak, nonpeak=nonpeak & ~peak, pitch=pitch, dpitch=dpitch, mag=mag, dmag=dmag)


def check_rows(got_pitch, got_mag, D, what=""):
    """Asserts the device's dense rows against decisions(): zeros at decided non-peaks, values within the bounds at decided peaks,
    anything at undecided entries. Returns (undecided entries, worst |d| / bound over the decided peaks)."""
    gp, gm = np.asarray(got_pitch, np.float64), np.asarray(got_mag, np.float64)
    assert gp.shape == D["peak"].shape == gm.shape, (what, gp.shape, D["peak"].shape)
    npk = D["nonpeak"]
    assert (gp[npk] == 0).all() and (gm[npk] == 0).all(), (what, "a decided non-peak holds a value", np.argwhere(npk & ((gp != 0) | (gm != 0)))[:4])
    pk = D["peak"]
    ep = np.abs(gp - D["pitch"])[pk] / D["dpitch"][pk]
    em = np.abs(gm - D["mag"])[pk] / D["dmag"][pk]
    assert (gp[pk] > 0).all(), (what, "a decided peak is missing", np.argwhere(pk & ~(gp > 0))[:4])
    ok = (ep <= 1.0) & (em <= 1.0)
    assert ok.all(), (what, int((~ok).sum()), np.argwhere(pk)[~ok][:4], float(ep.max()), float(em.max()))
    return int((~pk & ~npk).sum()), float(max(ep.max(initial=0.0), em.max(initial=0.0)))


NOTES = (57, 61, 64, 69)  # A3, C#4, E4, A4


def chord(T, sr, detune, seed=0, noise=1e-3):
    """The test input: four notes of three harmonics each (amplitudes 1, 1/2, 1/3, the sum scaled by 0.1), every note detuned by
    `detune` semitones from A440, plus seeded noise. float32 [T]."""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64) / sr
    y = np.zeros(T)
    for i, m in enumerate(NOTES):
        f0 = 440.0 * 2.0 ** ((m - 69 + detune) / 12.0)
        for h in (1, 2, 3):
            y += np.sin(2.0 * np.pi * h * f0 * t + 0.7 * i + 0.3 * h) / h
    return (0.1 * y + noise * rng.standard_normal(T)).astype(np.float32)


# The GPU grid (tests/test_gpu_tuning.py) and its CPU rehearsal (tests/test_tuning_cpu.py): (n_fft, hop_length, win_length, center), all at
# GRID_SR. The last takes the direct path. GRID_TILES: the frames a workgroup takes (vsyn_piptrack_tile, asserted on the CPU).
GRID_SR = 22050
GRID = [(2048, 512, 2048, True), (512, 128, 400, True), (64, 16, 64, False), (1102, 441, 1102, True)]
GRID_TILES = {GRID[0]: 1, GRID[1]: 4, GRID[2]: 32, GRID[3]: 8}
# The chord's detune on the grid. A partial that falls midway between two bins makes them tie, and a tie is undecided under any bound;
# the direct path's bound (K = win_length + 3) is some twenty times the FFT path's. At 0.23 the partial nearest to a midpoint in the
# 1102 framing is 0.068 bins from it; at 0.49 one is 0.001 bins from it, and those two bins tie in every frame.
GRID_DETUNE = 0.23


def grid_id(f):
    return "n%d_h%d_w%d_%s" % (f[0], f[1], f[2], "c" if f[3] else "nc")


def samples_for_frames(F, n_fft, hop, center):
    """A signal length that gives exactly F >= 1 frames."""
    T = (F - 1) * hop + (1 if center else n_fft)
    p = 2 * (n_fft // 2) if center else 0
    assert T + p >= n_fft and 1 + (T + p - n_fft) // hop == F
    return T


def grid_segments(framing):
    """The chord cut to frame counts 1, tile - 1, tile, tile + 1 and 2 tile + 1 (the distinct positive ones): float32 arrays."""
    n, hop, win, center = framing
    tile = GRID_TILES[framing]
    counts = sorted({F for F in (1, tile - 1, tile, tile + 1, 2 * tile + 1) if F >= 1})
    return [chord(samples_for_frames(F, n, hop, center), GRID_SR, GRID_DETUNE, seed=F) for F in counts]
