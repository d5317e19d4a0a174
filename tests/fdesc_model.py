"""The float64 model of the frame descriptor stage (include/vorbis_synth_hip.h, "frame descriptors", steps 1 to 10), written out step
by step from the header's words. It is the contract the device is compared against; tests/test_fdesc_cpu.py compares it against a
restatement with numpy.fft.rfft.

The DFT is a float64 matrix product with the header's twiddle table (numpy's cos and sin; the host's may differ in the last bit,
which `band` allows for); the sums over the bins and the frame energy are taken in np.longdouble and rounded once, as
tests/pitch_model.py does for its sums.

band, derived here and not tuned on the device, with u = 2^-53, N = n_fft, B = N / 2 + 1, V1 = sum_j |v_j| of the frame:
  S_k   One evaluation of re_k (or im_k) is a chain of N fused multiply-adds of terms bounded by |v_j|: at most N u V1 from the
        exact sum with its own table. Two tables differ by at most one ulp of a value below 1 per entry, 2 u V1 in the sum. Two
        evaluations differ by at most 2 (N + 1) u V1 per component, sqrt(2) times that in the magnitude, and 3 u S_k each for the
        squares, their sum and the root: e_k = 3 (N + 1) u V1 + 6 u S_k = e0 + 6 u S_k.
  rms   N non-negative terms, a division and a root, twice: 2 (N + 3) u.
  A     B terms, each off by e_k, summed in any order twice: dA = B e0 + (2 B + 6) u A. Every c_k is within dA as well.
  centroid   num = sum f_k S_k: dnum = e0 sum f_k + (2 B + 10) u num; band = dnum / num + dA / A + 2 u.
  bandwidth  W(c) = sum S_k (f_k - c)^2 = W(c*) + A (c - c*)^2 around the exact centroid c* (parallel axes), so two centroids
        within dc = band_centroid * centroid of each other move W by at most A (2 dc)^2; the rounding of f_k - c moves it by at
        most 2 u sr sqrt(A W) (Cauchy-Schwarz over the bins, f_k <= sr / 2, both sides); the S_k move it by e0 sum d_k^2:
        dW = e0 sum d_k^2 + 4 A dc^2 + 2 u sr sqrt(A W) + (2 B + 12) u W; band = (dW / W + dA / A) / 2 + 2 u.
  rolloff    theta = roll_percent A: dtheta = roll_percent dA + 2 u theta; a comparison c_k >= theta is decided alike by two
        evaluations when |c_k - theta| > dA + dtheta: band = ((1 + roll_percent) dA + 2 u theta) / theta, against
        margin = min_k |c_k - theta| / theta.
  flatness   dP_k = 2 S_k e_k + e_k^2 where (S_k + e_k)^2 > amin, else 0 (both sides clamp); dln_k = dP_k / max(amin,
        max(S_k - e_k, 0)^2). dL = mean dln_k + (2 B + 8) u mean |ln P_k| (a logarithm within one ulp, the sum, the division),
        dP = mean dP_k + (2 B + 4) u mean P_k; band = dL + dL^2 + dP / mean P_k + 8 u (the exponential within one ulp, the division).
zcr is an integer count over n_fft: exact, band 0."""
import numpy as np

U = 2.0 ** -53
TINY = 1.1754944e-38
COLS = 6
RMS, ZCR, CENTROID, BANDWIDTH, ROLLOFF, FLATNESS = range(6)


def num_frames(T, n, hop, center=True):
    """Step 1: the frame count of "spectral features" step 2."""
    if T == 0:
        return 0
    tp = T + (2 * (n // 2) if center else 0)
    return 0 if tp < n else 1 + (tp - n) // hop


def window(n, win):
    """Step 4: the spectral stage's window, float32 (n,)."""
    w = np.zeros(n, np.float32)
    i = np.arange(win, dtype=np.float64)
    w[(n - win) // 2:(n - win) // 2 + win] = (0.5 - 0.5 * np.cos(2.0 * np.pi * i / float(win))).astype(np.float32)
    return w


def twiddles(n):
    """Step 4: (cos, sin)(2.0 * pi * m / n), the angle evaluated left to right in double."""
    a = 2.0 * np.pi * np.arange(n, dtype=np.float64) / float(n)
    return np.cos(a), np.sin(a)


def frames_of(y, n, hop, center=True, edge=False):
    """Steps 2 and 3: the (F, n) float64 frames of the mono signal y (float32 values): zeros outside [0, T), or with edge=True the
    nearest valid sample."""
    y = np.asarray(y, np.float64)
    T = y.shape[0]
    F = num_frames(T, n, hop, center)
    if F == 0:
        return np.zeros((0, n), np.float64)
    t = np.arange(F, dtype=np.int64)[:, None] * hop - (n // 2 if center else 0) + np.arange(n, dtype=np.int64)[None, :]
    inside = (t >= 0) & (t < T)
    z = y[np.clip(t, 0, T - 1)]
    return z if edge else np.where(inside, z, 0.0)


def magnitudes(V):
    """Step 4 for frames V (F, n) of v_j: S (F, n / 2 + 1) float64."""
    F, n = V.shape
    B = n // 2 + 1
    c, s = twiddles(n)
    S = np.empty((F, B), np.float64)
    j = np.arange(n, dtype=np.int64)[:, None]
    step = max(1, (1 << 21) // n)
    for a in range(0, B, step):
        idx = (j * np.arange(a, min(a + step, B), dtype=np.int64)[None, :]) % n
        re, im = V @ c[idx], V @ s[idx]
        S[:, a:a + step] = np.sqrt(re * re + im * im)
    return S


def describe_many(signals, n, hop, win=None, center=True, roll=0.85, zthr=1e-10, amin=1e-10):
    """describe for a list of (y, sr): one DFT pass over the frames of all of them."""
    win = n if win is None else win
    w = window(n, win).astype(np.float64)
    B = n // 2 + 1
    outs, zs = [], []
    for y, sr in signals:
        y = np.asarray(y, np.float32)
        F = num_frames(y.shape[0], n, hop, center)
        out = dict(rows=np.zeros((F, COLS)), k=np.zeros(F, np.int64), margin=np.full(F, np.inf), band=np.zeros((F, COLS)), refused=False,
                   S=np.zeros((F, B)))
        if not np.isfinite(y).all():  # step 9
            out["refused"] = True
            out["rows"][:] = np.nan
            F = 0
        outs.append(out)
        zs.append(frames_of(y, n, hop, center) if F else np.zeros((0, n)))
    S_all = magnitudes(np.concatenate(zs) * w[None, :]) if sum(len(z) for z in zs) else np.zeros((0, B))
    at = 0
    for (y, sr), out, z in zip(signals, outs, zs):
        F = len(z)
        if F == 0:
            continue
        S = S_all[at:at + F]
        at += F
        out["S"] = S
        _fill(out, np.asarray(y, np.float32), float(sr), z, z * w[None, :], S, n, hop, center, roll, zthr, amin)
    return outs


def describe(y, sr, n=2048, hop=512, win=None, center=True, roll=0.85, zthr=1e-10, amin=1e-10):
    """Steps 1 to 10 on the mono signal y (T,) float32 at rate sr: dict(rows (F, 6) float64 before the rounding to float32, k (F,):
    k*, margin (F,): the roll-off margin, band (F, 6): the relative room per column (column 4: of the roll-off comparison),
    S (F, B), refused)."""
    return describe_many([(y, sr)], n, hop, win, center, roll, zthr, amin)[0]


def _fill(out, y, sr, z, V, S, n, hop, center, roll, zthr, amin):
    F, B = S.shape
    rows, band = out["rows"], out["band"]
    LD = np.longdouble
    # step 2
    rows[:, RMS] = np.sqrt((z.astype(LD) ** 2).sum(axis=1).astype(np.float64) / n)
    band[:, RMS] = 2 * (n + 3) * U
    # step 3
    ze = frames_of(y, n, hop, center, edge=True)
    s = (ze < 0.0) & (np.abs(ze) > zthr)
    rows[:, ZCR] = (s[:, 1:] != s[:, :-1]).sum(axis=1) / float(n)
    # steps 5 to 8
    fk = np.arange(B, dtype=np.float64) * sr / float(n)
    c = np.cumsum(S.astype(LD), axis=1).astype(np.float64)
    A = c[:, -1]
    num = (S.astype(LD) * fk[None, :]).sum(axis=1).astype(np.float64)
    live = A >= TINY
    As = np.where(live, A, 1.0)
    cent = np.where(live, num / As, 0.0)
    d = fk[None, :] - cent[:, None]
    W = (S.astype(LD) * d * d).sum(axis=1).astype(np.float64)
    rows[:, CENTROID] = cent
    rows[:, BANDWIDTH] = np.where(live, np.sqrt(W / As), 0.0)
    theta = roll * A
    k = np.argmax(c >= theta[:, None], axis=1)
    out["k"][:] = k
    rows[:, ROLLOFF] = k * sr / float(n)
    P = np.maximum(amin, S * S)
    lnP = np.log(P)
    Lbar = lnP.astype(LD).sum(axis=1).astype(np.float64) / B
    Pbar = P.astype(LD).sum(axis=1).astype(np.float64) / B
    rows[:, FLATNESS] = np.exp(Lbar) / Pbar
    # the band
    V1 = np.abs(V).sum(axis=1)
    e0 = 3.0 * (n + 1) * U * V1
    dA = B * e0 + (2 * B + 6) * U * A
    with np.errstate(divide="ignore", invalid="ignore"):
        dnum = e0 * fk.sum() + (2 * B + 10) * U * num
        bc = np.where(live & (num > 0), dnum / num + dA / A + 2 * U, 0.0)
        dc = bc * cent
        dW = e0 * (d * d).sum(axis=1) + 4 * A * dc * dc + 2 * U * sr * np.sqrt(A * W) + (2 * B + 12) * U * W
        bw = np.where(live & (W > 0), 0.5 * (dW / W + dA / A) + 2 * U, 0.0)
        br = np.where(theta > 0, ((1 + roll) * dA + 2 * U * theta) / theta, 0.0)
        out["margin"][:] = np.where(theta > 0, np.abs(c - theta[:, None]).min(axis=1) / theta, np.inf)
    ek = e0[:, None] + 6 * U * S
    dPk = np.where((S + ek) ** 2 > amin, 2 * S * ek + ek * ek, 0.0)
    dln = dPk / np.maximum(amin, np.maximum(S - ek, 0.0) ** 2)
    dL = dln.mean(axis=1) + (2 * B + 8) * U * np.abs(lnP).mean(axis=1)
    dP = dPk.mean(axis=1) + (2 * B + 4) * U * Pbar
    band[:, CENTROID] = bc
    band[:, BANDWIDTH] = bw
    band[:, ROLLOFF] = br
    band[:, FLATNESS] = dL + dL * dL + dP / Pbar + 8 * U
