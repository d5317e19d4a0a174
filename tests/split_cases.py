"""The inputs of the split stage's per-value test (tests/test_gpu_split.py, test 1): the (L, H), channel counts, lengths and nine
signals of tests/trim_cases.py by import, and three envelopes over the same noise whose silences lie INSIDE the signal.
tests/test_split_cpu.py asserts on the CPU that every one of them lies outside the band around the threshold."""
import numpy as np

from tests import trim_cases as tc
from tests import trim_model as tm
from tests.trim_cases import CHANNELS, LH, LOUD, QUIET, T_BIG, TOP_DB, lengths  # noqa: F401

EXTRA = ["bursts", "alternate", "last_frame"]
SIGNALS = tc.SIGNALS + EXTRA


def envelope(kind, T, L, H):
    """The amplitude of every sample, float32 (T,)."""
    if kind not in EXTRA:
        return tc.envelope(kind, T, L, H)
    env = np.full(T, QUIET, np.float32)
    if T == 0:
        return env
    if kind == "bursts":  # four loud stretches; the gap between the second and the third is L // 4 samples: shorter than a frame
        q = T // 9
        g = max(L // 4, 1)
        for a, b in ((q, 2 * q), (3 * q, 4 * q), (4 * q + g, 5 * q + g), (7 * q, 8 * q)):
            env[min(a, T):min(max(b, a + 1), T)] = LOUD
    elif kind == "alternate":  # loud in the first half-hop of every other frame's hop
        for f in range(0, tm.num_frames(T, L, H), 2):
            env[f * H:min(f * H + max(H // 2, 1), T)] = LOUD
    elif kind == "last_frame":  # an early burst, and the last L // 4 samples
        env[min(T // 8, T - 1):max(T // 4, 1)] = LOUD
        env[T - max(L // 4, 1):] = LOUD
    return env


def segment(case, kind, Cn, T, L, H):
    """One segment's (Cn, T) float32 PCM, as tests/trim_cases.py makes it."""
    if kind not in EXTRA:
        return tc.segment(case, kind, Cn, T, L, H)
    off = (case * 7919) % T_BIG
    return np.ascontiguousarray(tc._noise()[:Cn, off:off + T] * envelope(kind, T, L, H)[None, :], np.float32)


def cases(Cn, L, H):
    """Every (T, signal) of one (C, L, H): a list of (T, kind, x (Cn, T)). The first nine signals are trim_cases' own segments."""
    return [(T, kind, segment(ti * len(tc.SIGNALS) + si, kind, Cn, T, L, H)) if kind in tc.SIGNALS else
            (T, kind, segment(1000 + ti * len(EXTRA) + si, kind, Cn, T, L, H))
            for ti, T in enumerate(lengths(L, H)) for si, kind in enumerate(SIGNALS)]
