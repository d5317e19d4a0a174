"""Float64 model of the PCEN stage (include/vorbis_synth_hip.h, "PCEN", steps 1 to 4): the contract the device is tested against.
librosa.pcen(S.T * scale, sr, hop_length, gain, bias, power, time_constant, eps, b, max_size=1).T with the recurrence written as a
plain loop; tests/test_pcen_cpu.py checks it against scipy.signal.lfilter / lfilter_zi and librosa's three output expressions.
Also here: the parameter sets and inputs that the CPU and the GPU tests share, a NumPy restatement of the device's blocked order,
and the per-element gate."""
import numpy as np

U = 2.0 ** -24  # unit roundoff of float32
TINY = 2.0 ** -126  # a flushed denormal
BLK = 64  # rows per block of the device's scan

DEFAULTS = dict(gain=0.98, bias=2.0, power=0.5, time_constant=0.4, eps=1e-6, b=None, scale=1.0)

# the parameter sets of tests/test_pcen_cpu.py and tests/test_gpu_pcen.py
PARAMS = [
    dict(),
    dict(bias=0.0),
    dict(power=0.0),
    dict(gain=0.0),
    dict(b=1.0),
    dict(b=1e-4),
    dict(eps=1e-12, gain=0.8, bias=10.0, power=0.25),
]
SEG_ROWS = [37, 0, 1, 63, 64, 65, 128, 129, 1000]


def coefficient(time_constant, sr, hop_length):
    """Step 2: librosa's b for a time constant in seconds."""
    t = float(time_constant) * float(sr) / float(hop_length)
    return (np.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t)


def scaled(X, scale):
    """Step 1: S = float32(X * float32(scale)), as float32."""
    return (np.asarray(X, np.float32) * np.float32(scale)).astype(np.float32)


def smooth(S, b):
    """Step 3: M[f] = b S[f] + (1 - b) M[f-1], M[-1] = 1, per column, float64."""
    S = np.asarray(S, np.float64)
    M = np.empty_like(S)
    m = np.ones(S.shape[1:], np.float64)
    q = 1.0 - b
    for f in range(S.shape[0]):
        m = b * S[f] + q * m
        M[f] = m
    return M


def compress(S, M, gain, bias, power, eps):
    """Step 4, float64 (no rounding to float32)."""
    S = np.asarray(S, np.float64)
    with np.errstate(all="ignore"):
        G = np.exp(-gain * (np.log(eps) + np.log1p(M / eps)))
        if power == 0:
            return np.log1p(S * G)
        if bias == 0:
            return np.exp(power * (np.log(S) + np.log(G)))
        return bias ** power * np.expm1(power * np.log1p(S * G / bias))


def pcen64(X, sr=22050, hop_length=512, gain=0.98, bias=2.0, power=0.5, time_constant=0.4, eps=1e-6, b=None, scale=1.0):
    """The stage on one segment's rows X (F, D) in float64, before the last rounding."""
    X = np.asarray(X, np.float32)
    if b is None:
        b = coefficient(time_constant, sr, hop_length)
    S = scaled(X, scale)
    return compress(S, smooth(S, b), gain, bias, power, eps)


def pcen(X, **kw):
    """The stage on one segment's rows: float32 (F, D)."""
    with np.errstate(all="ignore"):
        return pcen64(X, **kw).astype(np.float32)


def blocked(X, sr=22050, hop_length=512, gain=0.98, bias=2.0, power=0.5, time_constant=0.4, eps=1e-6, b=None, scale=1.0):
    """The device's order in NumPy (parseoggvorbis_amd/csrc/vsyn_pcen.h): the zero-state response of every block of BLK rows but the
    last, the carries with q^BLK, then every block from its carry; float32 (F, D)."""
    X = np.asarray(X, np.float32)
    if b is None:
        b = coefficient(time_constant, sr, hop_length)
    q = 1.0 - b
    qblk = q ** BLK
    S = scaled(X, scale)
    F = S.shape[0]
    nblk = (F + BLK - 1) // BLK
    S64 = S.astype(np.float64)
    carry = [np.ones(S.shape[1:], np.float64)]
    for k in range(nblk - 1):
        m = np.zeros(S.shape[1:], np.float64)
        for f in range(k * BLK, (k + 1) * BLK):
            m = b * S64[f] + q * m
        carry.append(m + qblk * carry[k])
    M = np.empty_like(S64)
    for k in range(nblk):
        m = carry[k]
        for f in range(k * BLK, min((k + 1) * BLK, F)):
            m = b * S64[f] + q * m
            M[f] = m
    with np.errstate(all="ignore"):
        return compress(S, M, gain, bias, power, eps).astype(np.float32)


def rows(F, D, seed, scale=1.0):
    """Random non-negative float32 rows of a power spectrogram's spread (about eight decades) such that rows * scale is of the
    magnitude librosa's documentation feeds (2^31 x float PCM). Column 0 is zero throughout (D > 2); the last column (D > 1) falls
    silent from row 64 on."""
    rng = np.random.default_rng(seed)
    X = (10.0 ** rng.uniform(-4.0, 4.0, (F, D)) * (2.0 ** 31 / scale) * 1e-6).astype(np.float32)
    if D > 2:
        X[:, 0] = 0.0
    if D > 1:
        X[64:, D - 1] = 0.0
    return X


def gate(got, X, **kw):
    """The per-element gate of the issue on got (float32, what the device or a restatement returned) against the model on the same
    rows: |d| <= 2 u |Y| + 2^-126. One rounding to float32 (u |Y|), the float64 recurrence and library functions (terms that are
    non-negative, a few ulp of float64 each, conditioned by gain |log eps| < 30: below 2^-40 relative), and a flushed denormal.
    Returns the worst |d| / (u |Y|) over the elements with |Y| >= 2^-100; asserts for every element."""
    Y = pcen64(X, **kw)
    got = np.asarray(got, np.float32)
    assert got.shape == Y.shape, (got.shape, Y.shape)
    if Y.size == 0:
        return 0.0
    fin = np.isfinite(Y) & (np.abs(Y) <= np.finfo(np.float32).max)
    with np.errstate(all="ignore"):
        Y32 = Y.astype(np.float32)
    # where the model is not a finite float32 (only a NaN or an overflowing input gets there) the bits must be the model's
    assert np.array_equal(got[~fin], Y32[~fin], equal_nan=True)
    d = np.abs(got[fin].astype(np.float64) - Y[fin])
    bound = 2.0 * U * np.abs(Y[fin]) + TINY
    bad = d > bound
    assert not bad.any(), "%d of %d outside 2 u |Y| + 2^-126; worst |d| / (u |Y|) = %.3f" % (
        int(bad.sum()), d.size, float((d[bad] / (U * np.abs(Y[fin][bad]))).max()))
    big = np.abs(Y[fin]) >= 2.0 ** -100
    return float((d[big] / (U * np.abs(Y[fin][big]))).max()) if big.any() else 0.0
