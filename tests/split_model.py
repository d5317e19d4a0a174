"""The float64 model of the split stage (include/vorbis_synth_hip.h, "PCM splitting"): the trim stage's downmix, frame energies and
band (tests/trim_model.py, by import), the intervals and the joined signal. It is the contract the device is compared against;
tests/test_split_cpu.py compares it against a restatement in librosa's own words."""
import numpy as np

from tests.trim_model import AMIN_SQ, band, downmix, frame_ms  # noqa: F401


def loud_frames(ms, top_db):
    """Steps 2 and 3 of "PCM trimming": (mask (F,) bool, R, margin) of the frame energies ms."""
    F = ms.shape[0]
    R = max(float(ms.max()) if F else 0.0, AMIN_SQ)
    if F == 0:
        return np.zeros(0, bool), R, float("inf")
    thr = R * 10.0 ** (-float(top_db) / 10.0)  # one float64 product, as on the device
    E = np.maximum(ms, AMIN_SQ)
    return (E > thr) | (E >= R), R, float((np.abs(E - thr) / thr).min())


def split(y, top_db, L=2048, H=512):
    """The mono signal y (T,), float32 or float64: dict(intervals (n, 2) int64, joined (the concatenation of y[start:end]), R,
    ms (F,), margin). margin = min_f |E[f] - R k| / (R k) (inf with F = 0). A signal with a sample that is not finite is refused:
    no intervals, an empty joined signal, R not finite."""
    y = np.asarray(y)
    T = y.shape[0]
    none = np.zeros((0, 2), np.int64)
    if not np.isfinite(y).all():
        return dict(intervals=none, joined=y[:0], R=float("nan"), ms=None, margin=float("inf"))
    ms = frame_ms(y, L, H)
    mask, R, margin = loud_frames(ms, top_db)
    F = mask.shape[0]
    iv = []
    f = 0
    while f < F:  # maximal runs [a, b) of non-silent frames
        if not mask[f]:
            f += 1
            continue
        a = f
        while f < F and mask[f]:
            f += 1
        iv.append((a * H, min(f * H, T)))
    iv = np.asarray(iv, np.int64).reshape(-1, 2)
    joined = np.concatenate([y[a:b] for a, b in iv]) if len(iv) else y[:0]
    return dict(intervals=iv, joined=joined, R=R, ms=ms, margin=margin)


def joined_by_hops(y, mask, H):
    """The other form of the joined signal: the hops y[f H : min((f + 1) H, T)] of the non-silent frames f, in order."""
    T = y.shape[0]
    parts = [y[f * H:min((f + 1) * H, T)] for f in np.flatnonzero(mask)]
    return np.concatenate(parts) if parts else y[:0]
