"""Independent float64 model of the spectral features (include/vorbis_synth_hip.h, "spectral features"): numpy only, written from
the stated semantics (librosa's documented defaults), so that the GPU tests can compare the device against exact arithmetic."""
import math

import numpy as np


def hz_to_mel(f, htk=False):
    f = np.asarray(f, dtype=np.float64)
    if htk:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    with np.errstate(divide="ignore"):
        return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def mel_to_hz(m, htk=False):
    m = np.asarray(m, dtype=np.float64)
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filters(sr, n_fft, n_mels=128, fmin=0.0, fmax=None, htk=False, norm="slaney"):
    """W[n_mels][n_fft // 2 + 1] (librosa.filters.mel, in float64)."""
    fmax = sr / 2.0 if fmax is None else float(fmax)
    fk = np.arange(n_fft // 2 + 1, dtype=np.float64) * sr / n_fft
    hz = mel_to_hz(np.linspace(hz_to_mel(fmin, htk), hz_to_mel(fmax, htk), n_mels + 2), htk)
    W = np.zeros((n_mels, len(fk)))
    for m in range(n_mels):
        lower = (fk - hz[m]) / (hz[m + 1] - hz[m])
        upper = (hz[m + 2] - fk) / (hz[m + 2] - hz[m + 1])
        W[m] = np.maximum(0.0, np.minimum(lower, upper))
        if norm == "slaney":
            W[m] *= 2.0 / (hz[m + 2] - hz[m])
    return W


def window(n_fft, win_length=None):
    """Periodic Hann of win_length, zero-padded centred to n_fft."""
    win_length = n_fft if win_length is None else win_length
    i = np.arange(win_length, dtype=np.float64)
    w = np.zeros(n_fft)
    off = (n_fft - win_length) // 2
    w[off:off + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * i / win_length)
    return w


def support(n_fft, win_length=None):
    """bool [n_fft]: the window's support, [woff, woff + win_length) (a window value of 0 inside it included)."""
    win_length = n_fft if win_length is None else win_length
    j = np.arange(n_fft) - (n_fft - win_length) // 2
    return (j >= 0) & (j < win_length)


def num_frames(T, n_fft, hop_length, center=True):
    if T == 0:
        return 0
    tp = T + (2 * (n_fft // 2) if center else 0)
    return 0 if tp < n_fft else 1 + (tp - n_fft) // hop_length


def spectrum(x, n_fft=2048, hop_length=512, win_length=None, center=True, power=2.0):
    """S[frames][n_fft // 2 + 1] of planar PCM x[C][T] (or mono y[T])."""
    x = np.asarray(x, dtype=np.float64)
    y = x if x.ndim == 1 else x.mean(axis=0) if x.shape[0] > 1 else x[0]
    T = y.shape[0]
    F = num_frames(T, n_fft, hop_length, center)
    nb = n_fft // 2 + 1
    if F == 0:
        return np.zeros((0, nb))
    yp = np.pad(y, (n_fft // 2, n_fft // 2)) if center else y
    w = window(n_fft, win_length)
    idx = np.arange(F)[:, None] * hop_length + np.arange(n_fft)[None, :]
    frames = yp[idx] * w[None, :]
    frames[:, ~support(n_fft, win_length)] = 0.0  # a frame reads its window's support alone: an Inf or NaN outside it is not seen
    # the DFT as a matrix product in float64 (any n_fft), exact twiddles from (j * k) mod n_fft
    jk = np.outer(np.arange(n_fft), np.arange(nb)) % n_fft
    ang = 2.0 * np.pi * jk / n_fft
    re = frames @ np.cos(ang)
    im = frames @ np.sin(ang)
    mag2 = re * re + im * im
    return mag2 if power == 2 else np.sqrt(mag2)


def dct_ortho(n_mfcc, n_mels):
    """Rows of the orthonormal DCT-II: D[i][m] = sqrt((1 or 2) / N) cos(pi i (2m + 1) / 2N)."""
    i = np.arange(n_mfcc)[:, None]
    m = np.arange(n_mels)[None, :]
    D = np.sqrt(2.0 / n_mels) * np.cos(np.pi * i * (2 * m + 1) / (2.0 * n_mels))
    D[0] = np.sqrt(1.0 / n_mels)
    return D


def clamp_top_db(D, top_db):
    """Step 6's clamp of one segment's dB values: D = max(D, max of the segment's finite D - top_db). A value that is not finite
    (a frame that holds an Inf or NaN sample) takes no part in the maximum and stays as it is; top_db 0 or None: no clamp."""
    fin = np.isfinite(D)
    if not top_db or not fin.any():
        return D
    return np.where(fin, np.maximum(D, D[fin].max() - top_db), D)


def spectral(x, sr, kind="log_mel", n_fft=2048, hop_length=512, win_length=None, n_mels=128, fmin=0.0, fmax=None, htk=False,
             norm="slaney", center=True, power=2.0, log_floor=1e-3, amin=1e-10, top_db=80.0, n_mfcc=20):
    """The (frames, dim) matrix of one file in float64, plus the mel power M it was made from."""
    S = spectrum(x, n_fft, hop_length, win_length, center, power)
    M = S @ mel_filters(sr, n_fft, n_mels, fmin, fmax, htk, norm).T
    if kind == "mel_power":
        return M, M
    if kind == "log_mel":
        return np.log10(np.maximum(M, log_floor)), M
    D = 10.0 * np.log10(np.maximum(M, amin))
    D = clamp_top_db(D, top_db)
    if kind == "mel_db":
        return D, M
    return D @ dct_ortho(n_mfcc, n_mels).T, M
