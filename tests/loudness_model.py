"""Float64 model of the loudness stage (include/vorbis_synth_hip.h, "loudness", steps 1 to 5): the contract the device is tested
against. scipy.signal.lfilter per section, the integer hops, the gates and means, and every block's margin from both thresholds;
tests/test_loudness_cpu.py pins it to BS.1770-4's coefficient table, its 997 Hz calibration and EBU Tech 3341's cases 1 to 5.
Also here: the inputs the CPU and the GPU tests share, a NumPy restatement of the device's blocked order (chunks, Kogge-Stone scan
with the host's matrix powers, tile carries, apply), a sequential evaluation in np.longdouble, and the bound of DESIGN.md 6m."""
import math

import numpy as np
from scipy.signal import lfilter

U = 2.0 ** -53  # unit roundoff of float64
SUB, LANES, LEVELS = 32, 256, 8
TILE = SUB * LANES
MIN_RATE = 4000
Z_ABS = 10.0 ** ((-70.0 + 0.691) / 10.0)
OK, NOT_FINITE, TOO_SHORT, SILENT, RATE_REFUSED = 0, 1, 2, 3, 4
SECOND_ORDER = 1.0 + 2.0 ** -20  # the bounds are first order in U; what they leave out is below 2^-20 of them


# ---- step 1 ----
def coefficients(fs):
    """The ten coefficients in the device's order: b0 b1 b2 a1 a2 of the shelf, then of the high pass. Python floats: the operations
    of the header's formulas in the order the host library evaluates them."""
    fs = float(fs)
    G, Q, fc = 3.999843853973347, 0.7071752369554196, 1681.974450955533
    K = math.tan(math.pi * fc / fs)
    Vh = math.pow(10.0, G / 20.0)
    Vb = math.pow(Vh, 0.4996667741545416)
    a0 = 1.0 + K / Q + K * K
    k = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0,
         (1.0 - K / Q + K * K) / a0]
    Q, fc = 0.5003270373238773, 38.13547087602444
    K = math.tan(math.pi * fc / fs)
    a0 = 1.0 + K / Q + K * K
    return k + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]


def sections(fs):
    k = coefficients(fs)
    return (np.array(k[0:3]), np.array([1.0, k[3], k[4]])), (np.array(k[5:8]), np.array([1.0, k[8], k[9]]))


def kweight(x, fs):
    """x (..., T) -> the K-weighted signal, float64: lfilter per section from a zero state."""
    y = np.asarray(x, np.float64)
    for b, a in sections(fs):
        y = lfilter(b, a, y, axis=-1)
    return y


def downmix(x):
    """(C, T) float32 -> (1, T): the float32 expression of "PCM conditioning" step 1."""
    x = np.asarray(x, np.float32)
    s = x[0].copy()
    for c in range(1, x.shape[0]):
        s = s + x[c]
    return (s if x.shape[0] == 1 else s * (np.float32(1.0) / np.float32(x.shape[0])))[None, :].astype(np.float32)


# ---- step 2 ----
def num_hops(fs, T):
    return (10 * int(T)) // int(fs)


def hop_edges(fs, T):
    """Sample index of the start of hops 0 .. Nh (Nh + 1 numbers)."""
    return np.array([(i * int(fs)) // 10 for i in range(num_hops(fs, T) + 1)], np.int64)


def num_blocks(fs, T):
    return max(0, num_hops(fs, T) - 3) if fs >= MIN_RATE else 0


def lufs(zbar):
    return -0.691 + 10.0 * math.log10(zbar) if zbar > 0 else -math.inf


# ---- steps 2 to 5 ----
def measure(x, fs, target=None, mono=False, y=None):
    """x (C, T) float32. Returns a dict: status, y (Cs, T) float64, hops (Cs, Nh + 1) (the last the tail's), s (Nh,), n (block sample
    counts), z, keep_abs, keep_rel, zbar_a, zbar, blocks / blocks_abs / blocks_rel, lufs, gain (float32), margins (abs, rel):
    the smallest relative distance of a block from each threshold."""
    x = np.asarray(x, np.float32)
    if mono:
        x = downmix(x)
    T = x.shape[1]
    r = dict(status=OK, zbar=0.0, zbar_a=0.0, blocks=0, blocks_abs=0, blocks_rel=0, gain=np.float32(0.0), lufs=None, z=np.zeros(0))
    if fs < MIN_RATE:
        r["status"] = RATE_REFUSED
        return r
    finite = bool(np.isfinite(x).all())
    with np.errstate(all="ignore"):
        yw = kweight(x, fs) if y is None else y
    e = hop_edges(fs, T)
    Nh = len(e) - 1
    sq = yw * yw
    hops = np.zeros((x.shape[0], Nh + 1))
    for i in range(Nh):
        hops[:, i] = sq[:, e[i]:e[i + 1]].sum(axis=1)
    hops[:, Nh] = sq[:, e[Nh]:].sum(axis=1)
    r.update(y=yw, hops=hops, edges=e)
    Nb = max(0, Nh - 3)
    r["blocks"] = Nb
    s = hops[0, :Nh].copy()
    for c in range(1, x.shape[0]):
        s = s + hops[c, :Nh]
    n = np.array([e[j + 4] - e[j] for j in range(Nb)], np.float64)
    z = np.array([((s[j] + s[j + 1]) + s[j + 2]) + s[j + 3] for j in range(Nb)]) / n if Nb else np.zeros(0)
    r.update(s=s, n=n, z=z)
    if not finite:
        r["status"] = NOT_FINITE
        return r
    if Nb == 0:
        r["status"] = TOO_SHORT
        return r
    ka = z > Z_ABS
    r["keep_abs"] = ka
    r["blocks_abs"] = int(ka.sum())
    if not ka.any():
        r["status"] = SILENT
        r["lufs"] = -math.inf
        r["margins"] = (float(np.min(np.abs(z - Z_ABS) / Z_ABS)), math.inf)
        return r
    za = float(np.sum(z[ka]) / ka.sum())
    rel = za / 10.0
    kr = ka & (z > rel)
    zb = float(np.sum(z[kr]) / kr.sum())
    r.update(zbar_a=za, zbar=zb, keep_rel=kr, blocks_rel=int(kr.sum()), lufs=lufs(zb),
             margins=(float(np.min(np.abs(z - Z_ABS) / Z_ABS)), float(np.min(np.abs(z[ka] - rel) / rel))))
    if target is not None:
        r["gain"] = gain(zb, target)
    return r


def gain(zbar, target):
    """Step 4 from a zbar (the device's own, in the tests): float32(sqrt(Z_t / zbar))."""
    zt = math.pow(10.0, (float(target) + 0.691) / 10.0)
    return np.float32(np.sqrt(np.float64(zt) / np.float64(zbar)))


# ---- the device's order, restated ----
def transition(k):
    """The 4x4 matrix that takes the state (s1, s2, t1, t2) over one sample with x = 0, row-major list of 16."""
    return [-k[3], 1.0, 0.0, 0.0, -k[4], 0.0, 0.0, 0.0, k[6] - k[8] * k[5], 0.0, -k[8], 1.0, k[7] - k[9] * k[5], 0.0, -k[9], 0.0]


def matmul(a, b):
    """The host's 4x4 product: each element ((a0 b0 + a1 b1) + a2 b2) + a3 b3, Python floats."""
    return [((a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j]) + a[4 * i + 2] * b[8 + j]) + a[4 * i + 3] * b[12 + j] for i in range(4) for j in range(4)]


def powers(k):
    """A^(SUB 2^l), l = 0 .. LEVELS, each element the exact power correctly rounded to float64: A's elements are doubles, so 2^s A
    is an integer matrix and its powers are exact in Python integers. The host forms the same matrices in double-double arithmetic
    (tests/test_loudness_cpu.py holds its table to within U of the exact powers)."""
    key = tuple(k)
    if key in _POWERS:
        return _POWERS[key]
    from fractions import Fraction
    A = [Fraction(a) for a in transition(k)]
    s = max(a.denominator.bit_length() - 1 for a in A)
    Pi = [int(a * (1 << s)) for a in A]

    def sq(a):
        return [sum(a[4 * i + m] * a[4 * m + j] for m in range(4)) for i in range(4) for j in range(4)]
    n = 1
    while n < SUB:
        Pi, n = sq(Pi), 2 * n
    M = []
    for _ in range(LEVELS + 1):
        M.append([p / (1 << (s * n)) for p in Pi])  # (int / int is correctly rounded)
        Pi, n = sq(Pi), 2 * n
    _POWERS[key] = M
    return M


_POWERS = {}


def _step(v, k, x):
    y1 = k[0] * x + v[0]
    v0 = (v[1] + k[1] * x) - k[3] * y1
    v1 = k[2] * x - k[4] * y1
    y = k[5] * y1 + v[2]
    v2 = (v[3] + k[6] * y1) - k[8] * y
    v3 = k[7] * y1 - k[9] * y
    return [v0, v1, v2, v3], y


def _matvec_add(M, q, p):
    """p + M q on arrays of states (..., 4), in the device's order."""
    return np.stack([p[..., r] + (((M[4 * r] * q[..., 0] + M[4 * r + 1] * q[..., 1]) + M[4 * r + 2] * q[..., 2]) + M[4 * r + 3] * q[..., 3])
                     for r in range(4)], axis=-1)


def _run(chunks, k, v):
    """chunks (n, SUB) float64, v (n, 4): the cascade over every chunk at once. Returns (final states, outputs (n, SUB))."""
    v = [v[:, r].copy() for r in range(4)]
    ys = np.empty_like(chunks)
    for t in range(chunks.shape[1]):
        v, ys[:, t] = _step(v, k, chunks[:, t])
    return np.stack(v, axis=1), ys


def _scan(W, M):
    """Kogge-Stone over axis 1 of W (tiles, LANES, 4)."""
    for l in range(LEVELS):
        d = 1 << l
        W = np.concatenate([W[:, :d], _matvec_add(M[l], W[:, :-d], W[:, d:])], axis=1)
    return W


def blocked(x, fs):
    """One channel x (T,) float32 in the device's order: the K-weighted samples, float64 (T,)."""
    x = np.asarray(x, np.float32)
    T = len(x)
    if T == 0:
        return np.zeros(0)
    k = coefficients(fs)
    M = powers(k)
    tiles = -(-T // TILE)
    pad = np.zeros(tiles * TILE)
    pad[:T] = x
    chunks = pad.reshape(tiles * LANES, SUB)
    p, _ = _run(chunks, k, np.zeros((len(chunks), 4)))  # part: every lane from zero
    P = _scan(p.reshape(tiles, LANES, 4), M)[:, -1]
    carry = np.zeros((tiles, 4))
    for q in range(tiles - 1):
        carry[q + 1] = _matvec_add(M[LEVELS], carry[q], P[q])
    p0, _ = _run(chunks[::LANES], k, carry)  # apply: lane 0 of every tile from its carry
    W = p.reshape(tiles, LANES, 4).copy()
    W[:, 0] = p0
    W = _scan(W, M)
    start = np.concatenate([carry[:, None], W[:, :-1]], axis=1).reshape(-1, 4)
    _, ys = _run(chunks, k, start)
    return ys.reshape(-1)[:T]


def sequential_longdouble(x, fs):
    """One channel x (T,), the cascade sample by sample in np.longdouble with the coefficients of coefficients(fs)."""
    k = [np.longdouble(c) for c in coefficients(fs)]
    v = [np.longdouble(0)] * 4
    out = np.empty(len(x), np.longdouble)
    for t, xt in enumerate(np.asarray(x, np.float64)):
        v, out[t] = _step(v, k, np.longdouble(xt))
    return out


# ---- the bound ----
def _absmat(a):
    return np.abs(np.asarray(a, np.float64).reshape(4, 4))


_BOUNDS = {}


def bounds(fs):
    """Per unit of X = max |x|: dict(seq, dev): bounds on |y - y_exact| for the sequential float64 evaluation (the model) and for
    the device's blocked order, y_exact the cascade of the double coefficients in exact arithmetic. First order in U."""
    if fs in _BOUNDS:
        return _BOUNDS[fs]
    k = coefficients(fs)
    (b1, a1), (b2, a2) = sections(fs)
    N = max(4 * TILE, int(fs))
    d = np.zeros(N)
    d[0] = 1.0
    h1 = lfilter(b1, a1, d)
    Y1 = np.abs(h1).sum()
    Y = np.abs(lfilter(b2, a2, h1)).sum()
    ak = [abs(c) for c in k]
    S1, S2 = Y1 + ak[0], ak[2] + ak[4] * Y1
    T1, T2 = Y + ak[5] * Y1, ak[7] * Y1 + ak[9] * Y
    Sbar = np.array([S1, S2, T1, T2])
    e_y1 = U * (ak[0] + Y1)
    r_s1 = U * (ak[1] + (S2 + ak[1]) + ak[3] * Y1 + S1)
    r_s2 = U * (ak[2] + ak[4] * Y1 + S2)
    r_y = U * (ak[5] * Y1 + Y)
    r_t1 = U * (ak[6] * Y1 + (T2 + ak[6] * Y1) + ak[8] * Y + T1)
    r_t2 = U * (ak[7] * Y1 + ak[9] * Y + T2)
    A = np.array(transition(k)).reshape(4, 4)
    eta = np.array([ak[3] * e_y1 + r_s1, ak[4] * e_y1 + r_s2, abs(A[2, 0]) * e_y1 + ak[8] * r_y + r_t1, abs(A[3, 0]) * e_y1 + ak[9] * r_y + r_t2])
    e_out = ak[5] * e_y1 + r_y
    Cv = np.array([ak[5], 0.0, 1.0, 0.0])
    # |A^n| for n = 0 .. N - 1 (float64 products: the bound needs them to a few digits), and the sums and maxima over them
    Pn = np.empty((N, 4, 4))
    Pn[0] = np.eye(4)
    for n in range(1, N):
        Pn[n] = Pn[n - 1] @ A
    absP = np.abs(Pn)
    Sigma = absP.sum(axis=0)
    seq = float(Cv @ (Sigma @ eta) + e_out)
    # the matrices are within U |M_l| + 2^-1074 of the exact powers (one rounding, or a flush to zero); a product row of four terms
    # adds 4 U |M_l| |q|, the sum with p one more rounding of a state
    Mhost = powers(k)
    rho = [(5.0 * U * _absmat(Mhost[l]) + 2.0 ** -1074) @ Sbar + U * Sbar for l in range(LEVELS + 1)]
    # every event of the scan and of the tile chain goes to the output by one exact power: |C A^n| over the samples n between them
    rowC = np.abs(np.einsum("j,njk->nk", np.array([k[5], 0.0, 1.0, 0.0]), Pn))
    nb = N // SUB
    blk = rowC[:nb * SUB].reshape(nb, SUB, 4).max(axis=1)  # the maximum over a chunk's samples

    def reach(n, chunks):  # max |C A^n'| over n <= n' < n + SUB chunks (n a multiple of SUB); beyond N it is below 1e-100
        return blk[n // SUB:n // SUB + chunks].max(axis=0) if n // SUB < nb else np.zeros(4)
    scan = np.zeros(4)   # the events of the apply kernel's own scan, in front of this lane
    parts = np.zeros(4)  # those of the part kernel's scans in the tiles before, wherever this lane lies in its tile
    for l in range(LEVELS):
        for m in range(1 << (LEVELS - 1 - l)):
            n = SUB * m * (2 << l)
            scan += reach(n, 1) * rho[l]
            for j in range(nb * SUB // TILE + 1):
                parts += reach(n + TILE * j, LANES) * rho[l]
    chain = sum(reach(TILE * j, LANES) for j in range(nb * SUB // TILE + 1)) * rho[LEVELS]
    dev = float((scan + parts + chain).sum() + Cv @ (Sigma @ eta) + e_out)
    _BOUNDS[fs] = dict(seq=seq, dev=dev, norm1=float(Y), allpole=float(Sigma[2, 2]))
    return _BOUNDS[fs]


def sample_bound(fs, X):
    """The gate on |y_device - y_model| per sample for a channel with max |x| = X: both halves."""
    b = bounds(fs)
    return (b["seq"] + b["dev"]) * X * SECOND_ORDER


def block_bounds(m, fs, X):
    """From a measure() result m and X = max |x| over the measured signal: (Bz (Nb,), Bza, Bzbar): bounds on |z_j - z_j'|,
    |zbar_a - zbar_a'| and |zbar - zbar'| between the model and the device, given the same blocks are kept."""
    D = sample_bound(fs, X)
    ya = np.abs(m["y"])
    e = m["edges"]
    Nh = len(e) - 1
    Cs = ya.shape[0]
    Bs = np.zeros(Nh)
    for i in range(Nh):
        n = e[i + 1] - e[i]
        seg = ya[:, e[i]:e[i + 1]]
        d = (2.0 * seg * D + D * D).sum()
        Bs[i] = d + 2.0 * (n + 1) * U * (m["s"][i] + d)
    Nb = max(0, Nh - 3)
    Bz = np.array([(Bs[j:j + 4].sum()) / m["n"][j] + 2.0 * (Cs + 4) * U * m["z"][j] for j in range(Nb)]) * SECOND_ORDER
    out = [Bz]
    for keep, mean in ((m.get("keep_abs"), m["zbar_a"]), (m.get("keep_rel"), m["zbar"])):
        if keep is None or not keep.any():
            out.append(0.0)
        else:
            out.append(float(Bz[keep].mean() + 2.0 * (keep.sum() + 2) * U * mean))
    return tuple(out)


def margins_exceed(m, fs, X):
    """True when no block lies within its bound of a threshold: the device must then keep the model's blocks."""
    Bz, Bza, _ = block_bounds(m, fs, X)
    z = m["z"]
    if len(z) == 0:
        return True
    if not (np.abs(z - Z_ABS) > Bz).all():
        return False
    if m["status"] != OK:
        return True
    rel = m["zbar_a"] / 10.0
    ka = m["keep_abs"]
    return bool((np.abs(z[ka] - rel) > Bz[ka] + Bza / 10.0 + 2.0 * U * rel).all())


# ---- shared inputs ----
RATES = (8000, 11025, 48000)


def seg_lengths(fs):
    """The segment lengths of the stage tests at rate fs: the refusal edge, one block, the chunk and tile edges, a few seconds."""
    h4 = (4 * fs + 9) // 10  # the first T with four whole hops: (10 T) // fs >= 4
    return [0, h4 - 1, h4, h4 + 1, SUB - 1, SUB, SUB + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, int(2.3 * fs) + 7]


def signal(kind, C, T, seed):
    """(C, T) float32."""
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        return np.zeros((C, T), np.float32)
    x = 0.1 * rng.standard_normal((C, T))
    if kind == "dc":
        x = x + 0.5
    elif kind == "gated":  # loud (about -8 LUFS), 50 dB quieter (above the absolute gate, below the relative), digital zeros
        x = 3.0 * x
        a, b = T // 3, 2 * T // 3
        x[:, a:b] *= 10.0 ** (-50.0 / 20.0)
        x[:, b:] = 0.0
    return x.astype(np.float32)
