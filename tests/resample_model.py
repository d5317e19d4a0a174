"""Float64 model of the resampling contract (include/vorbis_synth_hip.h, "resampling"): scipy.signal.resample_poly with its
defaults, written out with its own I0, Kaiser window and sinc, no scipy. The device is tested against this."""
import math

import numpy as np

MAX_M = 65536


def ratio(r_in, r_out):
    g = math.gcd(int(r_in), int(r_out))
    return int(r_out) // g, int(r_in) // g


def valid(r_in, r_out):
    return r_in >= 1 and r_out >= 1 and max(ratio(r_in, r_out)) <= MAX_M


def num_frames(r_in, r_out, T):
    up, down = ratio(r_in, r_out)
    return -(-int(T) * up // down)


def i0(x):
    """Modified Bessel function of the first kind, order 0, by its power series (x may be an array)."""
    x = np.asarray(x, np.float64)
    q = 0.25 * x * x
    s = np.ones_like(x)
    t = np.ones_like(x)
    for k in range(1, 500):
        t = t * q / (k * k)
        s = s + t
        if np.all(t < 1e-17 * s):
            break
    return s


def taps(up, down):
    """h[0 .. N) in float64: up * w * sinc(m / M) / S."""
    M = max(up, down)
    H = 10 * M
    N = 2 * H + 1
    n = np.arange(N, dtype=np.float64)
    m = n - H
    r = 2.0 * n / (N - 1) - 1.0
    w = i0(5.0 * np.sqrt(np.maximum(0.0, 1.0 - r * r))) / i0(5.0)
    xs = np.pi * m / M
    sinc = np.where(m == 0, 1.0, np.sin(xs) / np.where(m == 0, 1.0, xs))
    h = w * sinc
    return up * h / h.sum()


def padded_taps(N, up):
    """K4 of step 3: the taps every phase reads, K = ceil(N / up) rounded up to a multiple of 4."""
    K = -(-N // up)
    return 4 * (-(-K // 4))


def polyphase(up, down, h=None):
    """P[phi][t] = h[phi + t up], t < K4 = K = ceil(N / up) rounded up to a multiple of 4 (step 3), zero past N. The padded taps add
    nothing to a finite signal; an Inf or NaN sample under one makes the sum NaN, as the header says."""
    h = taps(up, down) if h is None else h
    N = len(h)
    K = padded_taps(N, up)
    hp = np.zeros(K * up)
    hp[:N] = h
    return hp.reshape(K, up).T.copy()


def resample(x, r_in, r_out, h=None):
    """x: (T,) or (C, T) array; returns float64 (.., T_out). up == down returns x unchanged (as float64)."""
    x = np.asarray(x)
    up, down = ratio(r_in, r_out)
    if up == down:
        return x.astype(np.float64)
    xx = np.atleast_2d(x).astype(np.float64)
    T = xx.shape[-1]
    To = num_frames(r_in, r_out, T)
    P = polyphase(up, down, h)
    K = P.shape[1]
    M = max(up, down)
    H = 10 * M
    j = np.arange(To, dtype=np.int64)
    c = j * down + H
    phi, i0_ = c % up, c // up
    idx = i0_[:, None] - np.arange(K)[None, :]  # (To, K)
    ok = (idx >= 0) & (idx < T)
    w = P[phi]  # (To, K)
    out = np.zeros((xx.shape[0], To))
    for ch in range(xx.shape[0]):
        v = np.where(ok, xx[ch][np.clip(idx, 0, max(T - 1, 0))] if T else 0.0, 0.0)
        out[ch] = (w * v).sum(axis=1)
    return out[0] if x.ndim == 1 else out


def resample_at(x, r_in, r_out, j, P=None, block=1 << 22):
    """resample(x, r_in, r_out)[..., j] for a 1-D array of output indices j, by the same arithmetic (the same products, summed over
    the K axis in the same order), a block of rows at a time: for inputs and filters too long for the (T_out, K) arrays. P: the
    pair's polyphase(up, down), when the caller keeps it."""
    x = np.asarray(x)
    j = np.asarray(j, np.int64)
    up, down = ratio(r_in, r_out)
    if up == down:
        return x[..., j].astype(np.float64)
    xx = np.atleast_2d(x)
    T = xx.shape[-1]
    assert j.ndim == 1 and (not j.size or (j.min() >= 0 and j.max() < num_frames(r_in, r_out, T)))
    P = polyphase(up, down) if P is None else P
    K = P.shape[1]
    H = 10 * max(up, down)
    t = np.arange(K)[None, :]
    rows = max(1, block // K)
    out = np.zeros((xx.shape[0], j.size))
    for a in range(0, j.size, rows):
        c = j[a:a + rows] * down + H
        phi, i0_ = c % up, c // up
        idx = i0_[:, None] - t
        ok = (idx >= 0) & (idx < T)
        idx = np.clip(idx, 0, max(T - 1, 0))
        w = P[phi]
        for ch in range(xx.shape[0]):
            v = np.where(ok, xx[ch][idx].astype(np.float64) if T else 0.0, 0.0)
            out[ch, a:a + rows] = (w * v).sum(axis=1)
    return out[0] if x.ndim == 1 else out


def tap_index(r_in, r_out, j, p):
    """The index n = phi_j + (i0_j - p) up of the tap h[n] that output j applies to input sample p (step 3: y[j] = sum_t h[phi + t up]
    x[i0 - t], so t = i0 - p), or -1 where there is none: n outside [0, N). j and p broadcast; int64. Not for up == down."""
    up, down = ratio(r_in, r_out)
    M = max(up, down)
    H, N = 10 * M, 20 * M + 1
    c = np.asarray(j, np.int64) * down + H
    n = c % up + (c // up - np.asarray(p, np.int64)) * up
    return np.where((n >= 0) & (n < N), n, -1)
