"""The inputs of the frame descriptor stage's per-value tests (tests/test_gpu_fdesc.py), built in numpy from a fixed seed, shared with
tests/test_fdesc_cpu.py, which asserts on the CPU that every frame of every one of them decides its roll-off bin by a margin above
the band in which two float64 evaluations may disagree (tests/fdesc_model.py), and memoises the model's results for both.

Per (n_fft, hop, win_length): every signal at T = 4097, and the glide at every other length (T = 1: the click, whose one sample is
exact). Channels 1, 2, 3 and the rates 8000, 22050, 44100 rotate through the cases, so that a batch mixes rates."""
import functools

import numpy as np

from tests import fdesc_model as fm
from tests import pitch_cases as pc
from tests import trim_model as tm

CONFIGS = [(2048, 512, None), (512, 128, None), (64, 16, None), (16, 7, None), (1102, 441, None), (64, 200, None), (8192, 2048, None),
           (1024, 256, 700)]
CHANNELS = [1, 2, 3]
RATES = [8000, 22050, 44100]
SIGNALS = ["glide", "noise", "zeros", "click", "negative_dc", "alternating", "threshold"]
T_MID, T_BIG = 4097, 30011
ROLL, ZTHR, AMIN = 0.85, 1e-10, 1e-10


def lengths(n, hop):
    """T in {0, 1, hop-1, hop, n/2, n, 4097, 30011}, in that order."""
    return [0, 1, hop - 1, hop, n // 2, n, T_MID, T_BIG]


def segment(kind, Cn, T, sr, seed, n):
    """One segment's (Cn, T) float32 PCM: tests/pitch_cases.py's signals, and three of this stage's own, the same in every channel:
    negative_dc (every sample -0.25: edge padding gives zcr 0, zero padding would not), alternating (+0.3, -0.3, ..: zcr
    (n - 1) / n in interior frames), threshold (magnitudes 0.5e-10 and 2e-10 with mixed signs around zcr_threshold = 1e-10)."""
    if kind == "negative_dc":
        y = np.full(T, -0.25, np.float32)
    elif kind == "alternating":
        y = (0.3 * (1.0 - 2.0 * (np.arange(T) % 2))).astype(np.float32)
    elif kind == "threshold":
        rng = np.random.default_rng(20250914 + seed)
        y = (np.where(rng.random(T) < 0.5, 0.5e-10, 2e-10) * np.where(rng.random(T) < 0.5, -1.0, 1.0)).astype(np.float32)
    else:
        return pc.segment(kind, Cn, T, sr, seed, n)
    return np.ascontiguousarray(np.stack([y] * Cn), np.float32)


@functools.lru_cache(maxsize=None)
def cases(n, hop, win=None):
    """The cases of one configuration: a list of dict(kind, C, T, sr, x (C, T))."""
    todo = [(k, T_MID) for k in SIGNALS] + [("click" if T == 1 else "glide", T) for T in lengths(n, hop) if T != T_MID]
    out = []
    for k, (kind, T) in enumerate(todo):
        Cn = CHANNELS[k % 3]
        sr = RATES[(k + k // 3) % 3]
        out.append(dict(kind=kind, C=Cn, T=T, sr=sr, x=segment(kind, Cn, T, sr, CONFIGS.index((n, hop, win)) * 100 + k, n)))
    return out


def mono(c):
    return tm.downmix(c["x"]) if c["T"] else np.zeros(0, np.float32)


@functools.lru_cache(maxsize=None)
def models(n, hop, win=None):
    """tests/fdesc_model.py: describe of every case of the configuration, on the float32 downmix the device computes
    (tests/trim_model.py: downmix)."""
    return fm.describe_many([(mono(c), c["sr"]) for c in cases(n, hop, win)], n, hop, win, True, ROLL, ZTHR, AMIN)
