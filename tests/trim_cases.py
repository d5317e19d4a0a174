"""The inputs of the trim stage's per-value test (tests/test_gpu_trim.py, test 1), built in numpy, shared with tests/test_trim_cpu.py,
which asserts on the CPU that every one of them lies outside the band around the threshold in which two float64 evaluations may
disagree (tests/trim_model.py: band)."""
import functools

import numpy as np

from tests import trim_model as tm

LH = [(2048, 512), (400, 160), (64, 16), (7, 3), (1, 1), (16, 100), (8192, 2048)]
CHANNELS = [1, 2, 3]
TOP_DB = 60.0
LOUD, QUIET = np.float32(0.2), np.float32(1e-5)
SIGNALS = ["mid", "edge-1", "edge", "edge+1", "from_0", "last_hop", "zeros", "sub_amin", "one_sample"]
T_BIG = 100003


def lengths(L, H):
    """T in {0, 1, 2, H-1, H, H+1, L//2, L, 4097, 100003}, in that order (duplicates kept: each is a case of its own)."""
    return [0, 1, 2, H - 1, H, H + 1, L // 2, L, 4097, T_BIG]


@functools.lru_cache(maxsize=None)
def _noise():
    return np.random.default_rng(20240917).standard_normal((max(CHANNELS), 2 * T_BIG)).astype(np.float32)


def envelope(kind, T, L, H):
    """The amplitude of every sample, float32 (T,)."""
    env = np.full(T, QUIET, np.float32)
    if T == 0:
        return env
    F = tm.num_frames(T, L, H)
    if kind == "mid":  # noise at 0.2 between a lead-in and a tail of noise at 1e-5
        env[T // 3 + 1:2 * T // 3 + 1] = LOUD
    elif kind.startswith("edge"):  # the loud part starts one sample before, at, one sample after the end of frame F // 3
        e = min(max((F // 3) * H - L // 2 + L + {"edge-1": -1, "edge": 0, "edge+1": 1}[kind], 0), T - 1)
        env[e:max(e + 1, 2 * T // 3)] = LOUD
    elif kind == "from_0":  # loud from t = 0: start = 0
        env[:2 * T // 3 + 1] = LOUD
    elif kind == "last_hop":  # loud only in the last partial hop: end = T by the clamp
        env[(T - 1) // H * H:] = LOUD
    elif kind == "zeros":
        env[:] = 0.0
    elif kind == "sub_amin":
        env[:] = 1e-6
    elif kind == "one_sample":
        env[:] = 0.0
    else:
        raise ValueError(kind)
    return env


def segment(case, kind, Cn, T, L, H):
    """One segment's (Cn, T) float32 PCM: every channel its own noise under the envelope; case picks the stretch of noise."""
    off = (case * 7919) % T_BIG
    x = _noise()[:Cn, off:off + T] * envelope(kind, T, L, H)[None, :]
    if kind == "one_sample" and T:
        x[:, T // 2] = np.float32(0.5)
    return np.ascontiguousarray(x, np.float32)


def cases(Cn, L, H):
    """Every (T, signal) of one (C, L, H): a list of (T, kind, x (Cn, T))."""
    return [(T, kind, segment(ti * len(SIGNALS) + si, kind, Cn, T, L, H)) for ti, T in enumerate(lengths(L, H)) for si, kind in enumerate(SIGNALS)]
