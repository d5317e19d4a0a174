"""Float64 model of the PCM conditioning stage (include/vorbis_synth_hip.h, "PCM conditioning"): mono downmix, peak normalisation,
pre-emphasis. The arithmetic is written out here, step by step as the header numbers it; the device is compared against this, not
against librosa or RETURNN (neither is a test dependency). The pre-emphasis is checked against scipy.signal.lfilter in
tests/test_condition_cpu.py."""
import numpy as np


def downmix(x):
    """Step 1: y[t] = the mean of the channels, x (C, T) -> (T,)."""
    x = np.asarray(x, np.float64)
    assert x.ndim == 2 and x.shape[0] >= 1
    return x.sum(axis=0) / x.shape[0]


def peak(y):
    """Step 2: p = max |y| (0 for T = 0)."""
    y = np.asarray(y, np.float64)
    return float(np.abs(y).max()) if y.size else 0.0


def peak_normalize(y):
    """Step 2: y / p when p > 0, y otherwise; a peak that is not finite is refused."""
    y = np.asarray(y, np.float64)
    p = peak(y)
    if not np.isfinite(p):
        raise ValueError("the peak is not finite")
    return y / p if p > 0.0 else y.copy()


def coefficient(a):
    """Step 3: the coefficient rounded once to float32, as a float64."""
    return float(np.float32(a))


def preemphasis(y, a):
    """Step 3: z[0] = y[0], z[t] = y[t] - a32 y[t-1]."""
    y = np.asarray(y, np.float64)
    z = y.copy()
    z[1:] -= coefficient(a) * y[:-1]
    return z


def condition(x, peak_normalization=False, a=None):
    """The stage: x (C, T) -> z (T,), in the order downmix, peak, pre-emphasis."""
    y = downmix(x)
    if peak_normalization:
        y = peak_normalize(y)
    return preemphasis(y, a) if a is not None else y
