"""Inputs shared by tests/test_beat_cpu.py (which asserts that each one decides every comparison of the beat tracker by more than the
band two correct float64 evaluations can disagree in, tests/beat_model.py) and tests/test_gpu_beat.py (which runs them on the
device). The shapes are the smallest at which the kernels take another path: B = lo frames a step, a ring of 2P + B values, 64
candidates a lane round, 256 frames a score tile."""
import functools

import numpy as np

from tests import beat_model as bm
from tests import rhythm_model as rm

PERIODS = (1, 2, 3, 5, 7, 64, 65, 2048)  # 5 and 7: h = 2 and 4 (half to even); 1: lo = max(h, 1)


def lengths(P):
    """The lengths run at one P: two and three frames, around lo, around the ring's wrap (2P, 2P + 1), a partial last step (2P + B + 1), 600
    and 4097 (those >= 2; F = 1 and F = 0 are cases of their own)."""
    lo = bm.half(P)[1]
    return sorted(set(F for F in (2, 3, lo - 1, lo, lo + 1, 2 * P, 2 * P + 1, 2 * P + lo + 1, 600, 4097) if F >= 2))


def _train(F, P, seed):
    """Clicks a period apart over a little noise; P <= 2 has no room between clicks, a random envelope stands in."""
    if P <= 2:
        return (rm.envelope(F, seed) + np.float32(0.5)).astype(np.float32)
    return rm.click_train(F=F, period=P, first=min(P // 3, F - 1), noise=0.01, seed=seed)


def _plateau(F=300):
    """For P = 1: stretches of exact zeros wider than the window. ls is an exact 0 inside them and cum[i] = cum[i - 1] there in any
    evaluation (tx[1] = 0), so the frame in front of a stretch is a local maximum by the >= of the rule alone and the frames inside it
    are none by its >."""
    x = (rm.envelope(F, 21) + np.float32(0.5)).astype(np.float32)
    x[100:110] = 0.0
    x[200:204] = 0.0
    x[F - 5:] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def cases():
    """A tuple of (name, envelope, P, tightness, trim)."""
    out = []
    for P in PERIODS:
        for F in lengths(P):
            out.append(("P%d_F%d" % (P, F), _train(F, P, 1000 * P + F), P, 100.0, True))
    for P, F in ((7, 600), (20, 600), (64, 600)):
        for tight in (1.0, 400.0):
            out.append(("P%d_F%d_tight%g" % (P, F, tight), _train(F, P, 7 * P + F), P, tight, True))
        out.append(("P%d_F%d_untrimmed" % (P, F), _train(F, P, 7 * P + F), P, 100.0, False))
    out.append(("clicks20", rm.click_train(), 20, 100.0, True))
    out.append(("clicks37", rm.click_train(F=900, period=37, first=11), 37, 100.0, True))
    out.append(("random_P11", rm.envelope(500, 3), 11, 100.0, True))
    out.append(("random_P11_even", rm.envelope(503, 4), 11, 100.0, True))
    out.append(("plateau", _plateau(), 1, 100.0, True))
    out.append(("plateau_untrimmed", _plateau(), 1, 100.0, False))
    out.append(("late_start", rm.click_train(F=400, period=20, first=150, noise=0.001, seed=5), 20, 100.0, True))  # i0 far from 0
    # sd = 0: a constant whose sums are exact; u = x / FLT_MIN. (With candidates and P > 1 a constant ties structurally, frame after
    # frame, in sums that are equal only in exact arithmetic: no evaluation decides those, so the constants here are P = 1, where the
    # window is one frame wide and cum counts the frames exactly, and F < lo.)
    out.append(("constant", np.full(300, FLT_MIN32, np.float32), 1, 100.0, True))
    out.append(("constant_one", np.full(300, 1.0, np.float32), 1, 100.0, True))
    out.append(("constant_below_lo", np.full(9, FLT_MIN32, np.float32), 20, 100.0, True))
    out.append(("below_lo", rm.envelope(31, 5), 64, 100.0, True))  # F < lo: never a candidate
    out.append(("zeros", np.zeros(50, np.float32), 7, 100.0, True))
    out.append(("one_frame", np.ones(1, np.float32), 7, 100.0, True))
    out.append(("no_frames", np.zeros(0, np.float32), 7, 100.0, True))
    out.append(("many_steps", rm.click_train(F=20000, period=22, first=7, noise=0.01, seed=9), 22, 100.0, True))
    return tuple(out)


FLT_MIN32 = np.float32(np.finfo(np.float32).tiny)


def names():
    return [c[0] for c in cases()]


def case(name):
    return next(c for c in cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def model(name):
    """The model's result for one case, computed once a process and left unchanged."""
    _, x, P, tight, trim = case(name)
    return bm.beat_track(x, P, tight, trim)


def mixed_batch():
    """(names, periods): several cases in one call, a refused (NaN) segment and a skipped (P = 0) one among them."""
    picks = ["clicks20", "P5_F11", "nan", "P2048_F4097", "skipped", "plateau", "zeros", "late_start", "P1_F600", "one_frame", "clicks20", "P64_F600", "no_frames"]
    return picks


def batch_segment(name):
    """(envelope, P, tightness, trim) of a mixed_batch entry."""
    if name == "nan":
        x = rm.envelope(70, 8)
        x[64] = np.nan
        return x, 7, 100.0, True
    if name == "skipped":
        return rm.envelope(40, 9), 0, 100.0, True
    return case(name)[1:]
