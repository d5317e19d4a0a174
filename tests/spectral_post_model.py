"""Float64 model of the spectral post-processing stage (include/vorbis_synth_hip.h, "spectral post-processing"): the delta /
delta-delta columns of librosa.feature.delta (scipy.signal.savgol_filter(..., deriv=o, polyorder=o, mode="interp")) in closed form,
and per-column mean / mean-variance normalisation. Plain numpy."""
import numpy as np


def delta_coefs(width, order):
    """c_o[k], k = -h .. h, as float64 (order 1 or 2)."""
    assert width % 2 == 1 and width >= 3 and order in (1, 2)
    h = (width - 1) // 2
    k = np.arange(-h, h + 1, dtype=np.float64)
    s2, s4 = (k ** 2).sum(), (k ** 4).sum()
    if order == 1:
        return k / s2
    return 2.0 * (width * k ** 2 - s2) / (width * s4 - s2 * s2)


def delta(x, width=9, order=1, coefs=None):
    """D_o of x (F, D): interior rows sum_k c[k] x[f + k], the h rows at either end repeat the first / last interior row.
    coefs overrides the coefficients (e.g. their float32 roundings)."""
    x = np.asarray(x, dtype=np.float64)
    F = x.shape[0]
    if F == 0:
        return x.copy()
    if F < width:
        raise ValueError("width %d must not exceed the number of frames %d" % (width, F))
    c = delta_coefs(width, order) if coefs is None else np.asarray(coefs, dtype=np.float64)
    h = (width - 1) // 2
    inner = np.zeros((F - 2 * h,) + x.shape[1:])
    for i in range(width):  # k ascending
        inner += c[i] * x[i:i + F - 2 * h]
    idx = np.clip(np.arange(F), h, F - 1 - h) - h
    return inner[idx]


def with_deltas(x, order=0, width=9):
    """Y = [X | D_1 | D_2] up to order."""
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([x] + [delta(x, width, o) for o in range(1, order + 1)], axis=1)


def stats(y):
    """Per-column mu and population sigma of y (F, D_out), F > 0."""
    mu = y.mean(axis=0)
    return mu, np.sqrt(((y - mu) ** 2).mean(axis=0))


def normalize(y, norm=None, given=None, std_floor=1e-5):
    """norm None / "mean" / "mean_var" with the segment's own statistics, or given = (mean, std) (std None: mean only)."""
    y = np.asarray(y, dtype=np.float64)
    if given is not None:
        mu = np.asarray(given[0], dtype=np.float64)
        sigma = None if given[1] is None else np.asarray(given[1], dtype=np.float64)
    elif norm is None or y.shape[0] == 0:
        return y
    else:
        mu, sigma = stats(y)
        if norm == "mean":
            sigma = None
        else:
            assert norm == "mean_var", norm
    z = y - mu
    return z if sigma is None else z / np.maximum(sigma, std_floor)


def post(x, delta=0, delta_width=9, normalize_=None, std_floor=1e-5):
    """The whole stage with the keyword semantics of get_spectral_batch: normalize_ None, "mean", "mean_var" or (mean, std)."""
    y = with_deltas(x, delta, delta_width)
    if isinstance(normalize_, tuple):
        return normalize(y, given=normalize_, std_floor=std_floor)
    return normalize(y, normalize_, std_floor=std_floor)
