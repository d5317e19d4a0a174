"""The inputs of the pitch stage's per-value tests (tests/test_gpu_pitch.py), built in numpy from a fixed seed, shared with
tests/test_pitch_cpu.py, which asserts on the CPU that every frame of every one of them decides its lag by a margin above the band
in which two float64 evaluations may disagree (tests/pitch_model.py: band), and memoises the model's results for both.

Per (L, H): every signal at T = 4097, and the glide at every other length (T = 1: the click, whose one sample is exact). Channels
1, 2, 3 and the rates 8000, 22050, 44100 rotate through the cases, so that a batch mixes p_min and p_max."""
import functools

import numpy as np

from tests import pitch_model as pm
from tests import trim_model as tm

LH = [(2048, 512), (512, 128), (64, 16), (8, 2), (8192, 2048)]
CHANNELS = [1, 2, 3]
RATES = [8000, 22050, 44100]
SIGNALS = ["glide", "periodic", "zeros", "noise", "quiet_glide", "onset", "click"]
T_MID, T_BIG = 4097, 30011
THRESHOLD = 0.1
LOUD = ("glide", "periodic", "noise", "onset")  # compared against the restatement in librosa's words


def lengths(L, H):
    """T in {0, 1, H-1, H, L/2, L, 4097, 30011}, in that order."""
    return [0, 1, H - 1, H, L // 2, L, T_MID, T_BIG]


def band_hz(L, sr):
    """fmin and fmax of the cases: p_min = 2, 5, 11 at the three rates, and p_max past L - L/2 - 1 at 44100 Hz (the clamp) and below it
    at 8000; for L = 8 the only lags there are, 2 and 3."""
    if L < 64:
        return sr / 8.0, sr / 2.0
    return 44100.0 * 0.55 / (L // 2 - 1), min(sr / 2.0, 4000.0)


def signal(kind, T, sr, seed, L):
    """One channel's (T,) float32."""
    rng = np.random.default_rng(20250301 + seed)
    t = np.arange(T, dtype=np.float64)
    if kind in ("glide", "quiet_glide", "onset"):
        # a three-harmonic glide with vibrato, a period near L/16 samples that grows by 3 % over the segment, noise at 0.01
        p0 = max(L / 16.0, 2.0) + 1.37
        period = p0 * (1.0 + 0.03 * t / max(T, 1)) + 0.003 * p0 * np.sin(2 * np.pi * 5.0 * t / sr)
        ph = 2 * np.pi * np.cumsum(1.0 / period)
        y = 0.5 * np.sin(ph) + 0.25 * np.sin(2 * ph + 0.3) + 0.125 * np.sin(3 * ph + 1.1) + 0.01 * rng.standard_normal(T)
        if kind == "quiet_glide":
            y *= 1e-5
        if kind == "onset":  # silence up to the middle of a frame
            y[:T // 2 + min(L // 3, T // 4)] = 0.0
        return y.astype(np.float32)
    if kind == "periodic":  # an exactly periodic float32 pattern of integer period
        P = max(L // 8, 3)
        return np.tile(rng.uniform(-0.7, 0.7, P).astype(np.float32), T // P + 1)[:T]
    if kind == "zeros":
        return np.zeros(T, np.float32)
    if kind == "noise":
        return (0.3 * rng.standard_normal(T)).astype(np.float32)
    if kind == "click":  # a single non-zero sample; 0.5 in every channel, so that the downmix is 0.5 exactly
        y = np.zeros(T, np.float32)
        if T:
            y[T // 2] = 0.5
        return y
    raise ValueError(kind)


def segment(kind, Cn, T, sr, seed, L):
    """One segment's (Cn, T) float32 PCM: the channels differ in their noise (and the periodic pattern in its values), not in period."""
    return np.ascontiguousarray(np.stack([signal(kind, T, sr, seed * 4 + c if kind != "click" else 0, L) for c in range(Cn)]), np.float32)


@functools.lru_cache(maxsize=None)
def cases(L, H):
    """The cases of one (L, H): a list of dict(kind, C, T, sr, fmin, fmax, x (C, T))."""
    todo = [(k, T_MID) for k in SIGNALS] + [("click" if T == 1 else "glide", T) for T in lengths(L, H) if T != T_MID]
    out = []
    for k, (kind, T) in enumerate(todo):
        Cn = CHANNELS[k % 3]
        sr = 8000 if (T == T_BIG and L >= 2048) else RATES[(k + k // 3) % 3]  # (the long case of the long frames at the rate with the fewest lags)
        fmin, fmax = band_hz(L, sr)
        out.append(dict(kind=kind, C=Cn, T=T, sr=sr, fmin=fmin, fmax=fmax, x=segment(kind, Cn, T, sr, LH.index((L, H)) * 100 + k, L)))
    return out


@functools.lru_cache(maxsize=None)
def models(L, H):
    """tests/pitch_model.py: yin of every case of (L, H), on the float32 downmix the device computes (tests/trim_model.py: downmix)."""
    return [pm.yin(tm.downmix(c["x"]) if c["T"] else np.zeros(0, np.float32), c["sr"], c["fmin"], c["fmax"], L, H, THRESHOLD, True) for c in cases(L, H)]
