"""The inputs of the pyin stage's per-value tests (tests/test_gpu_pyin.py), built in numpy from fixed seeds on the signals of
tests/pitch_cases.py, shared with tests/test_pyin_cpu.py, which asserts on the CPU that every discrete decision of every one of
them is decided (tests/pyin_model.py), and memoises the model's results for both.

Groups share one spec (one launch each on the device), and mix channels 1, 2, 3 and two rates:
    default   (2048, 512), C2 to C7, the defaults at 22050 Hz: B = 601, w = 101 (44100 Hz: w = 51). An octave jump (vp == 1 frames,
              back pointers that leave the band), zeros and the click (no trough, all-equal unvoiced values), noise (the most troughs,
              frames with h >= 1 everywhere: only the no-trough term), the exactly periodic pattern (h = 0 < t_1), every short length.
    narrow    (512, 128), 200 to 280 Hz: B = 59; at 8000 Hz w = 71 > B (no out-of-band state), at 16000 Hz w = 31. T = 30011 for the
              decode's length.
    small     (64, 16), resolution 0.5: B = 12, w = 3.
    coarse    (2048, 512), 30 to 60 Hz, resolution 0.5: two bins a semitone at lags of 367 to 735, so that several troughs share a
              bin and the last one wins. (The section's check wants 0 < resolution < 1, so 0.5 is the coarsest grid there is.)
    top       (512, 128) at 8000 Hz, fmax = 8000 / 20: a tone of period 20 lands on bin == B and is dropped; a tone just below fmin
              is clipped to bin 0.
"""
import functools

import numpy as np

from tests import pitch_cases as pc
from tests import pyin_model as ym
from tests import trim_model as tm

C2, C7 = 65.40639132514966, 2093.004522404789
N_THRESHOLDS = 100
GROUPS = {
    "default": dict(L=2048, H=512, fmin=C2, fmax=C7, resolution=0.1),
    "narrow": dict(L=512, H=128, fmin=200.0, fmax=280.0, resolution=0.1),
    "small": dict(L=64, H=16, fmin=400.0, fmax=550.0, resolution=0.5),
    "coarse": dict(L=2048, H=512, fmin=30.0, fmax=60.0, resolution=0.5),
    "top": dict(L=512, H=128, fmin=150.0, fmax=400.0, resolution=0.1),
}
T_MID = 4097


def tone(T, sr, freqs, seed, noise=0.003):
    """A three-harmonic tone whose frequency steps through freqs in equal parts, with a little noise."""
    rng = np.random.default_rng(20260101 + seed)
    f = np.repeat(np.asarray(freqs, np.float64), -(-T // len(freqs)))[:T]
    ph = 2 * np.pi * np.cumsum(f / sr)
    y = 0.5 * np.sin(ph) + 0.2 * np.sin(2 * ph + 0.3) + 0.1 * np.sin(3 * ph + 1.1) + noise * rng.standard_normal(T)
    return y.astype(np.float32)


def _segment(kind, Cn, T, sr, seed, L, arg):
    if kind == "tone":
        return np.ascontiguousarray(np.stack([tone(T, sr, arg, seed * 4 + c) for c in range(Cn)]), np.float32)
    return pc.segment(kind, Cn, T, sr, seed, L)


def _plan():
    """(group, kind, C, T, sr, argument of the signal)"""
    out = []
    L, H = 2048, 512
    out += [("default", "tone", 1, 3 * T_MID, 22050, (220.0, 440.0, 220.0)), ("default", "zeros", 2, T_MID, 44100, None),
            ("default", "click", 3, T_MID, 22050, None), ("default", "noise", 2, T_MID, 22050, None),
            ("default", "periodic", 1, T_MID, 44100, None), ("default", "glide", 3, 0, 22050, None), ("default", "click", 1, 1, 44100, None),
            ("default", "glide", 2, H - 1, 22050, None), ("default", "glide", 1, L, 44100, None)]
    L, H = 512, 128
    out += [("narrow", "tone", 1, pc.T_BIG, 8000, (210.0, 270.0, 215.0, 265.0, 240.0)), ("narrow", "tone", 2, T_MID, 16000, (230.0, 260.0)),
            ("narrow", "noise", 3, T_MID, 8000, None), ("narrow", "zeros", 1, H - 1, 16000, None), ("narrow", "glide", 2, L, 8000, None)]
    L, H = 64, 16
    out += [("small", "tone", 1, T_MID, 8000, (402.0, 530.0)), ("small", "noise", 2, 3 * L, 11025, None), ("small", "click", 3, T_MID // 4, 8000, None),
            ("small", "tone", 2, L, 11025, (500.0,)), ("small", "glide", 1, H - 1, 8000, None)]
    out += [("coarse", "noise", 1, T_MID, 22050, None), ("coarse", "tone", 2, T_MID, 22050, (29.8, 45.0)), ("coarse", "tone", 3, T_MID, 44100, (50.0, 33.0))]
    out += [("top", "tone", 1, T_MID, 8000, (400.0,)), ("top", "tone", 2, T_MID, 8000, (149.5, 300.0)), ("top", "noise", 3, 2 * 512, 8000, None)]
    return out


@functools.lru_cache(maxsize=None)
def beta():
    from parseoggvorbis_amd.pitch import beta_probs
    return beta_probs(N_THRESHOLDS, (2, 18))


@functools.lru_cache(maxsize=None)
def cases():
    """A list of dict(group, kind, C, T, sr, x (C, T), and the group's L, H, fmin, fmax, resolution)."""
    out = []
    for k, (grp, kind, Cn, T, sr, arg) in enumerate(_plan()):
        g = GROUPS[grp]
        out.append(dict(g, group=grp, kind=kind, C=Cn, T=T, sr=sr, x=_segment(kind, Cn, T, sr, 700 + k, g["L"], arg)))
    return out


def run_model(c, y=None):
    y = (tm.downmix(c["x"]) if c["T"] else np.zeros(0, np.float32)) if y is None else y
    return ym.pyin(y, c["sr"], c["fmin"], c["fmax"], beta(), c["L"], c["H"], resolution=c["resolution"])


@functools.lru_cache(maxsize=None)
def models():
    """tests/pyin_model.py: pyin of every case, on the float32 downmix the device computes (tests/trim_model.py: downmix)."""
    return [run_model(c) for c in cases()]
