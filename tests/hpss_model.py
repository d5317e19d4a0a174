"""Float64 model of the HPSS stage (include/vorbis_synth_hip.h, "HPSS", steps 1 to 3): the contract the device is tested against.
librosa.decompose.hpss(S.T, kernel_size=(kh, kp), power, mask, margin=(margin_h, margin_p)) transposed, with the two median filters
written as an explicit reflected gather and a selection; tests/test_hpss_cpu.py checks the medians against numpy.pad + sort and
scipy.ndimage.median_filter, and the masks against librosa.util.softmask in librosa's own words. Also here: the parameter sets and
inputs that the CPU and the GPU tests share, and the per-element gate."""
import numpy as np

U = 2.0 ** -24  # unit roundoff of float32
TINY = 2.0 ** -126  # a flushed denormal; also FLT_MIN, the threshold of a "bad" element

KERNELS = [(1, 1), (3, 3), (31, 31), (63, 63), (5, 17), (17, 5)]
POWERS = [1.0, 2.0, 0.5, np.inf]
MARGINS = [(1.0, 1.0), (2.0, 1.0), (1.0, 3.0)]
COMPONENTS = ["harmonic", "percussive"]
OUTPUTS = ["component", "mask", "median"]
SEG_ROWS = [1, 2, 3, 30, 31, 32, 63, 64, 65, 200]
DIMS = [1, 2, 17, 128, 257, 1025]


def reflect(i, n):
    """Step 1's index rule, numpy.pad(mode="symmetric") as often as needed: i mod 2n, and 2n - 1 - that when it is >= n."""
    m = np.mod(np.asarray(i, np.int64), 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


def median(X, k, axis):
    """Step 1: the element of rank k // 2 of the k reflected neighbours along axis, float32 in and out. A window that holds a NaN
    gives NaN (numpy orders NaNs last, so the window's largest element tells)."""
    X = np.asarray(X, np.float32)
    assert k % 2 == 1 and X.ndim == 2
    n = X.shape[axis]
    idx = reflect(np.arange(n)[:, None] + np.arange(-(k // 2), k // 2 + 1)[None, :], n)  # (n, k)
    W = np.partition(np.take(X, idx, axis=axis), (k // 2, k - 1), axis=axis + 1)  # axis 0: (n, k, D); axis 1: (F, n, k)
    med, top = np.take(W, k // 2, axis=axis + 1), np.take(W, k - 1, axis=axis + 1)
    return np.where(np.isnan(top), np.float32(np.nan), med).astype(np.float32)


def softmask(A, B, power, split_zeros):
    """Step 2 in float64: A and B are float64 arrays (B already times its margin)."""
    with np.errstate(all="ignore"):
        if np.isinf(power):
            return (A > B).astype(np.float64)
        Z = np.maximum(A, B)
        bad = Z < TINY
        Zs = np.where(bad, 1.0, Z)
        a, b = (A / Zs) ** power, (B / Zs) ** power
        return np.where(bad, 0.5 if split_zeros else 0.0, a / (a + b))


def medians(X, kernel_size):
    """(H, P) of step 1 as float32."""
    return median(X, kernel_size[0], 0), median(X, kernel_size[1], 1)


def hpss64(X, component="harmonic", kernel_size=(31, 31), power=2.0, margin=(1.0, 1.0), output="component", HP=None):
    """The stage on one segment's rows X (F, D) in float64, before the last rounding (the median output: the float32 medians).
    HP: medians(X, kernel_size) where the caller has them already."""
    X = np.asarray(X, np.float32)
    kh, kp = kernel_size
    mh, mp = margin
    if output == "median":
        if HP is not None:
            return HP[0 if component == "harmonic" else 1].astype(np.float64)
        return (median(X, kh, 0) if component == "harmonic" else median(X, kp, 1)).astype(np.float64)
    H, P = (a.astype(np.float64) for a in (HP if HP is not None else medians(X, kernel_size)))
    split = mh == 1 and mp == 1
    with np.errstate(all="ignore"):
        M = softmask(H, P * mh, power, split) if component == "harmonic" else softmask(P, H * mp, power, split)
        return M if output == "mask" else X.astype(np.float64) * M


def hpss(X, **kw):
    """The stage on one segment's rows: float32 (F, D)."""
    with np.errstate(all="ignore"):
        return hpss64(X, **kw).astype(np.float32)


def rows(F, D, seed):
    """Random non-negative float32 rows that run every branch: about sixteen decades of dynamic range, a band of columns quantised
    to four values (many ties), a band of exact zeros (digital silence: the FLT_MIN branch), a band of denormals, and a few loud rows
    (a percussive event) and a loud column (a harmonic one)."""
    rng = np.random.default_rng(seed)
    X = (10.0 ** rng.uniform(-8.0, 8.0, (F, D))).astype(np.float32)
    c = np.arange(D)
    X[:, c % 8 == 1] = np.float32(0.25) * rng.integers(0, 4, (F, int((c % 8 == 1).sum()))).astype(np.float32)  # ties, zeros among them
    X[:, c % 8 == 2] = 0.0
    X[:, c % 8 == 3] = (rng.integers(0, 1 << 20, (F, int((c % 8 == 3).sum()))).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    r = np.arange(F)
    X[r % 16 == 5] *= np.float32(64.0)
    X[r % 32 == 9] = 0.0  # silent rows: zeros on both sides of every mask there
    X[:, c % 16 == 12] *= np.float32(64.0)
    return X


def gate(got, X, **kw):
    """The per-element gate of the issue on got (float32, what the device returned) against the model on the same rows. Component and
    mask: |d| <= 2 u |Y| + 2^-126: one rounding to float32 (u |Y|) and a flushed denormal; the float64 quotient, power and a + b are
    sums and ratios of non-negative terms, a few ulp of float64, and every decision (max, Z < FLT_MIN, A > B) is exact on float32
    medians and one correctly rounded product. Median: equality as values (-0 == +0), NaN where the model has NaN. Returns the worst
    |d| / (u |Y|) over the elements with |Y| >= 2^-100 (0 for the median output); asserts for every element."""
    Y = hpss64(X, **kw)
    got = np.asarray(got, np.float32)
    assert got.shape == Y.shape, (got.shape, Y.shape)
    if Y.size == 0:
        return 0.0
    if kw.get("output", "component") == "median":
        assert np.array_equal(np.isnan(got), np.isnan(Y))
        ok = ~np.isnan(Y)
        assert np.array_equal(got[ok].astype(np.float64), Y[ok]), "%d medians differ" % int((got[ok].astype(np.float64) != Y[ok]).sum())
        return 0.0
    fin = np.isfinite(Y) & (np.abs(Y) <= np.finfo(np.float32).max)
    with np.errstate(all="ignore"):
        Y32 = Y.astype(np.float32)
    # where the model is not a finite float32 (only a non-finite input gets there) the value must be the model's
    assert np.array_equal(got[~fin], Y32[~fin], equal_nan=True)
    d = np.abs(got[fin].astype(np.float64) - Y[fin])
    bound = 2.0 * U * np.abs(Y[fin]) + TINY
    bad = d > bound
    assert not bad.any(), "%d of %d outside 2 u |Y| + 2^-126; worst |d| / (u |Y|) = %.3f" % (
        int(bad.sum()), d.size, float((d[bad] / (U * np.abs(Y[fin][bad]) + 1e-300)).max()))
    big = np.abs(Y[fin]) >= 2.0 ** -100
    return float((d[big] / (U * np.abs(Y[fin][big]))).max()) if big.any() else 0.0
