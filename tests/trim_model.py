"""The float64 model of the trim stage (include/vorbis_synth_hip.h, "PCM trimming", steps 1 to 7), written out step by step. It is
the contract the device is compared against; tests/test_trim_cpu.py compares it against a restatement in librosa's own words.

Frame sums are taken per frame in np.longdouble (64-bit mantissa here) over a strided view of the zero-padded squares: the terms
are non-negative, so the sum's relative error is at most L * 2^-64, 2^-11 of the device's one float64 chain; one rounding to
float64 follows. A cumulative sum would not do: the difference of two prefix sums loses a quiet frame behind a loud passage.
tests/test_trim_cpu.py checks the sums against math.fsum."""
import math

import numpy as np

AMIN_SQ = 1e-10  # librosa's amin = 1e-5 on the amplitude, squared


def downmix(x):
    """Step 1 as the device computes it: the float32 sum of the channels in ascending order, times float32(1 / C) when C > 1.
    x (C, T) float32 -> (T,) float32."""
    x = np.asarray(x, np.float32)
    s = x[0].copy()
    for c in range(1, x.shape[0]):
        s = s + x[c]
    return s if x.shape[0] == 1 else s * (np.float32(1.0) / np.float32(x.shape[0]))


def num_frames(T, L, H):
    """Step 2: librosa's frame count under center=True."""
    if T == 0 or T + 2 * (L // 2) - L < 0:
        return 0
    return 1 + (T + 2 * (L // 2) - L) // H


def frame_ms(y, L, H):
    """Step 2: ms[f] = (1 / L) sum_{i < L} y[f H - L // 2 + i]^2 with zeros outside [0, T), float64 (F,)."""
    y = np.asarray(y)
    T = y.shape[0]
    F = num_frames(T, L, H)
    if F == 0:
        return np.zeros(0, np.float64)
    sq = (y.astype(np.float64) ** 2).astype(np.longdouble)  # exact for float32 input
    half = L // 2
    need = (F - 1) * H + L  # padded samples the F frames span
    pad = np.zeros(max(need, half + T), np.longdouble)
    pad[half:half + T] = sq
    frames = np.lib.stride_tricks.sliding_window_view(pad, L)[::H][:F]
    return (frames.sum(axis=1) / np.longdouble(L)).astype(np.float64)


def frame_ms_fsum(y, L, H, f):
    """One frame of step 2 with math.fsum (exactly rounded sum), for the model's own check."""
    T = len(y)
    lo, hi = max(0, f * H - L // 2), min(T, f * H - L // 2 + L)
    return math.fsum(float(v) * float(v) for v in y[max(lo, 0):max(hi, 0)]) / L


def trim(y, top_db, L=2048, H=512):
    """Steps 2 to 5 on the mono signal y (T,), float32 or float64: dict(start, end, ms (F,), R, margin). margin =
    min_f |E[f] - R k| / (R k): the distance of the closest frame from the threshold (inf with F = 0). A signal with a sample that
    is not finite is refused (step 6): start = end = 0, R not finite, margin inf."""
    y = np.asarray(y)
    T = y.shape[0]
    if not np.isfinite(y).all():
        return dict(start=0, end=0, ms=None, R=float("nan"), margin=float("inf"))
    ms = frame_ms(y, L, H)
    F = ms.shape[0]
    R = max(float(ms.max()) if F else 0.0, AMIN_SQ)
    if F == 0:
        return dict(start=0, end=0, ms=ms, R=R, margin=float("inf"))
    k = 10.0 ** (-float(top_db) / 10.0)
    thr = R * k  # one float64 product, as on the device
    E = np.maximum(ms, AMIN_SQ)
    loud = np.flatnonzero((E > thr) | (E >= R))  # (E >= R: a loudest frame, also where R k rounds to R)
    f0, f1 = int(loud[0]), int(loud[-1])
    margin = float((np.abs(E - thr) / thr).min())
    return dict(start=f0 * H, end=min(T, (f1 + 1) * H), ms=ms, R=R, margin=margin)


def band(L):
    """The distance from the threshold inside which two float64 evaluations of E[f] > R k may disagree: each of ms[f] and R carries
    at most (L + 1) roundings of 2^-53 (one chain of L non-negative terms and the division), the product one more."""
    return (2 * L + 3) * 2.0 ** -53
