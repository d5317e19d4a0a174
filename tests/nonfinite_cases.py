"""What one Inf or NaN value does in every stage that reads PCM or rows: the footprints, written from the formulas of
include/vorbis_synth_hip.h alone (never from a kernel's constants), and the batches, positions and comparisons that
tests/test_nonfinite_cpu.py (the float64 models) and tests/test_gpu_nonfinite.py (the device) share.

The one test shape. A batch of S = 3 segments of seeded noise, of different lengths, each plane NaN behind its segment's frames. A
clean run and a dirty run, the dirty batch being the clean one with a value v (NaN, +Inf, -Inf) written into segment 1, one channel.
Outside the footprint the dirty output equals the clean one bit for bit; inside it no value is finite."""
import math

import numpy as np

from tests import resample_model as rm
from tests import spectral_model as sm

VALUES = {"nan": np.float32(np.nan), "+inf": np.float32(np.inf), "-inf": np.float32(-np.inf)}
DIRTY_SEG, DIRTY_CH = 1, 1  # the segment (of 3) and the channel (of 2, or 0 of 1) that receives the value
LDS_BYTES = 160 * 1024  # gfx950: LDS of one workgroup, what the tile formulas below divide up


# ---- footprints ----

def spectral_footprint(samples, T, n_fft, hop, win_length=None, center=True):
    """bool [F]: the frames whose window support [f hop - pad + woff, f hop - pad + woff + win_length) holds one of `samples`
    ("spectral features", step 8)."""
    win = n_fft if win_length is None else win_length
    pad, woff = (n_fft // 2 if center else 0), (n_fft - win) // 2
    lo = np.arange(sm.num_frames(T, n_fft, hop, center), dtype=np.int64) * hop - pad + woff
    hit = np.zeros(lo.shape, bool)
    for s in samples:
        assert 0 <= s < T
        hit |= (lo <= s) & (s < lo + win)
    return hit


def resample_footprint(samples, T, r_in, r_out):
    """bool [T_out]: the outputs j one of whose K4 taps x[i0 - t], t < K4, is one of `samples` ("resampling", step 3)."""
    up, down = rm.ratio(r_in, r_out)
    To = rm.num_frames(r_in, r_out, T)
    if up == down:
        hit = np.zeros(To, bool)
        hit[list(samples)] = True
        return hit
    M = max(up, down)
    H, N = 10 * M, 20 * M + 1
    K4 = rm.padded_taps(N, up)
    i0 = (np.arange(To, dtype=np.int64) * down + H) // up
    hit = np.zeros(To, bool)
    for s in samples:
        assert 0 <= s < T
        hit |= (i0 - K4 + 1 <= s) & (s <= i0)
    return hit


def delta_rows(f, F, width):
    """bool [F]: the rows r of D_o that read row f: |clamp(r, h, F-1-h) - f| <= h ("spectral post-processing", steps 1 and 5)."""
    h = (width - 1) // 2
    assert F >= width and 0 <= f < F
    return np.abs(np.clip(np.arange(F), h, F - 1 - h) - f) <= h


def post_footprint(f, d, F, D, order, width, segment_stats):
    """bool [F][D (1 + order)] for a value at X[f][d]: Y[f][d], the delta rows that read row f in the columns D + d, 2 D + d, and with
    the segment's own statistics every row of those columns."""
    hit = np.zeros((F, D * (1 + order)), bool)
    hit[f, d] = True
    for o in range(1, order + 1):
        hit[delta_rows(f, F, width), o * D + d] = True
    if segment_stats:
        hit[:, d::D] = True
    return hit


def pcen_footprint(f, d, F, D):
    """bool [F][D]: rows >= f of column d, where the smoother M of "PCEN" step 3 is not finite. For a NaN and a -Inf Y is not finite
    there either (rule 7); for +Inf see pcen_plus_inf."""
    hit = np.zeros((F, D), bool)
    hit[f:, d] = True
    return hit


def pcen_plus_inf(f, d, F, D):
    """(not finite, forced) bool [F][D] for a +Inf with gain > 0 (rule 7): row f is NaN; behind it M = +Inf makes the gain G = 0, so
    Y is step 4's value at G = 0 there, a 0 for every form of the compression."""
    nf, forced = np.zeros((F, D), bool), np.zeros((F, D), bool)
    nf[f, d] = True
    forced[f + 1:, d] = True
    return nf, forced


# ---- tiles: how many frames one workgroup takes, from the LDS images that the header and DESIGN.md state ----

def mel_lds_floats(ft, n_fft, hop, n_mels):
    """spec_lds_floats: twiddles 2 n | window n | span (ft - 1) hop + n | |X|^power ft x 256 | M ft x n_mels."""
    return 3 * n_fft + (ft - 1) * hop + n_fft + ft * 256 + ft * n_mels


def mel_tile(n_fft, hop, n_mels):
    for ft in (16, 4, 1):
        if 4 * mel_lds_floats(ft, n_fft, hop, n_mels) <= LDS_BYTES:
            return ft
    return 0


def lin_tile(n_fft, hop):
    """vsyn_spectral_lin_tile restated: 2048 / n_fft frames (at most 64, at least 1) for a power of two; else 8 frames of the direct
    loop if twiddles, window and span fit the LDS, else 1."""
    if n_fft & (n_fft - 1) == 0:
        return 1 if n_fft >= 2048 else min(64, 2048 // n_fft)
    for ft in (8, 1):
        if 4 * (3 * n_fft + (ft - 1) * hop + n_fft) <= LDS_BYTES:
            return ft
    return 0


# ---- batches and positions ----

def pcm_batch(lengths, channels, seed, plane=None, burst=None):
    """(pcm float32 [S][C][plane], frames int32 [S]): seeded noise of amplitude 0.3, NaN behind each segment's frames. burst =
    (start, length): segment 1 is near-silent (1e-6) outside a loud stretch (x 30) there, which spans more than 80 dB."""
    rng = np.random.default_rng(seed)
    plane = max(lengths) + 5 if plane is None else plane
    pcm = np.full((len(lengths), channels, plane), np.nan, np.float32)
    for g, T in enumerate(lengths):
        x = 0.3 * rng.standard_normal((channels, T))
        if burst is not None and g == DIRTY_SEG:
            x *= 1e-6 / 0.3
            x[:, burst[0]:burst[0] + burst[1]] = 9.0 * rng.standard_normal((channels, burst[1]))
        pcm[g, :, :T] = x.astype(np.float32)
    return pcm, np.asarray(lengths, np.int32)


def dirtied(pcm, writes, ch=None):
    """A copy of the batch with writes = [(t, value), ...] put into segment 1, one channel."""
    out = pcm.copy()
    c = min(DIRTY_CH, pcm.shape[1] - 1) if ch is None else ch
    for t, v in writes:
        out[DIRTY_SEG, c, t] = v
    return out


def spectral_positions(T, n_fft, hop, win_length, center, tile):
    """name -> samples of segment 1 (T frames): t = 0; t = T - 1 (without centring: behind the last whole frame, T is chosen so);
    the first sample of frame `tile`'s support (or sample 0 where that lies in the padding), which the last frame of the workgroup
    tile before it covers too; and a pair inside
    one frame for +Inf / -Inf."""
    win = n_fft if win_length is None else win_length
    pad, woff = (n_fft // 2 if center else 0), (n_fft - win) // 2
    F = sm.num_frames(T, n_fft, hop, center)
    assert F > tile and hop < win, (F, tile)
    s_tile = max(tile * hop - pad + woff, 0)
    fp = spectral_footprint([s_tile], T, n_fft, hop, win_length, center)
    assert fp[tile - 1] and fp[tile] and not fp.all()
    mid = (F // 2) * hop - pad + woff + win // 2
    pos = {"first": [0], "last": [T - 1], "tile": [s_tile], "pair": [mid, mid + 1]}
    if not center:
        assert (T - n_fft) % hop >= 1 and not spectral_footprint([T - 1], T, n_fft, hop, win_length, center).any()
        pos["behind"] = pos.pop("last")
        pos["last"] = [(F - 1) * hop + woff + win - 1]  # the last sample that a frame covers
    return pos


def writes_of(name, samples, vname):
    """The values for a position: one value; the pair takes +Inf and -Inf whatever vname says."""
    if name == "pair":
        return [(samples[0], VALUES["+inf"]), (samples[1], VALUES["-inf"])]
    return [(s, VALUES[vname]) for s in samples]


def cases(positions):
    """(position, value name) pairs: every single position with each of the three values, the pair once."""
    return [(p, v) for p in positions for v in (VALUES if p != "pair" else ["+inf"])]


# ---- comparisons ----

def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_footprint(clean, dirty, hit, what, complex_values=False):
    """clean, dirty float32 of one shape, hit a bool mask of that shape (complex_values: of half the last axis, a value being a pair
    re, im): equal bits where hit is false, and where it is true no dirty value finite and every clean value finite (else the
    case shows nothing)."""
    clean, dirty = np.asarray(clean), np.asarray(dirty)
    assert clean.dtype == dirty.dtype == np.float32 and clean.shape == dirty.shape, (what, clean.shape, dirty.shape)
    if complex_values:
        c, d = clean.view(np.complex64), dirty.view(np.complex64)
        assert c.shape == hit.shape, (what, c.shape, hit.shape)
        same = np.repeat(~hit, 2, axis=-1)
    else:
        c, d, same = clean, dirty, ~hit
        assert c.shape == hit.shape, (what, c.shape, hit.shape)
    diff = same & (bits(clean) != bits(dirty))
    assert not diff.any(), (what, "changed outside the footprint", int(diff.sum()), np.argwhere(diff)[:4])
    fin = hit & np.isfinite(d)
    assert not fin.any(), (what, "finite inside the footprint", int(fin.sum()), np.argwhere(fin)[:4], d[fin][:4])
    assert np.isfinite(c[hit]).all(), (what, "the clean run is not finite there")


def fma32(a, b, c):
    """float32 fma(a, b, c) elementwise, correctly rounded: the product is exact in float64, the sum is rounded to odd there (the
    error of the float64 sum, by TwoSum, decides), and rounding that to float32 is then the single rounding of the exact value
    (53 >= 2 * 24 + 2 bits)."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    odd = (s.view(np.int64) & 1) != 0
    fix = (e != 0) & ~odd & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def dct32(n_mfcc, n_mels):
    """The device's DCT-II table: float32 of sqrt((1 or 2) / N) cos(pi i (2m + 1) / 2N) evaluated in double."""
    return np.array([[math.sqrt((2.0 if i else 1.0) / n_mels) * math.cos(math.pi * i * (2.0 * m + 1.0) / (2.0 * n_mels))
                      for m in range(n_mels)] for i in range(n_mfcc)]).astype(np.float32)


def mfcc32(D, n_mfcc):
    """out[r][i] = sum_m dct[i][m] D[r][m] as one float32 fma chain, m ascending ("spectral features", MFCC of clamped dB rows)."""
    D = np.asarray(D, np.float32)
    c = dct32(n_mfcc, D.shape[1])
    acc = np.zeros((D.shape[0], n_mfcc), np.float32)
    for m in range(D.shape[1]):
        acc = fma32(c[None, :, m], D[:, m, None], acc)
    return acc


def clamp32(D0, keep, top_db):
    """The header's rule for top_db in float32: the maximum of the finite D0 (top_db = 0 rows) over the rows `keep`, minus top_db, and
    D = that where D0 is below it. Returns float32 of D0's shape (only the rows `keep` mean anything)."""
    D0 = np.asarray(D0, np.float32)
    if not top_db:
        return D0.copy()
    thr = np.float32(D0[keep].max()) - np.float32(top_db)
    return np.where(D0 < thr, thr, D0).astype(np.float32)


def s16(x):
    """VSYN_PCM_S16 restated: round-to-nearest-even of the float32 product x * 32768, clamped to [-32768, 32767]; a NaN gives -32768."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(x, np.float32) * np.float32(32768.0)).astype(np.float64)
    r = np.where(np.isnan(r), -32768.0, np.clip(r, -32768.0, 32767.0))
    return r.astype(np.int16)


S16_INPUTS = np.array([np.nan, np.inf, -np.inf, 1.0, -1.0, 65536.0, -65536.0, np.finfo(np.float32).max, -np.finfo(np.float32).max,
                       np.nextafter(np.finfo(np.float32).max, np.float32(0)), 0.25, -0.75], np.float32)
S16_WANT = np.array([-32768, 32767, -32768, 32767, -32768, 32767, -32768, 32767, -32768, 32767, 8192, -24576], np.int16)


# ---- the shapes: (n_fft, hop, win_length, center, lengths of the three segments, frames per workgroup) ----
# Without centring segment 1's length leaves a tail behind its last whole frame ((T - n_fft) % hop >= 1).

LIN_SHAPES = [
    (64, 16, 64, True, [300, 645, 410], 32),            # FFT kernel, many frames per tile
    (64, 16, 40, False, [300, 711, 410], 32),           # win_length < n_fft: woff = 12, so t = 0 lies in frame 0 but outside its support
    (2048, 512, 2048, True, [1100, 2660, 2100], 1),     # FFT kernel, one frame per tile, six frames
    (96, 24, 96, True, [200, 483, 300], 8),             # direct kernel, 8 frames per tile
    (6000, 2500, 6000, False, [6100, 13509, 8600], 1),  # direct kernel whose 8-frame image does not fit the LDS
]
LIN_KINDS = [("stft", {}), ("lin_power", dict(power=1)), ("lin_power", dict(power=2)), ("lin_db", dict(power=2, top_db=None))]

MEL_SR, N_MELS, N_MFCC = 16000, 8, 6
MEL_SHAPES = [
    (64, 16, 64, True, [300, 645, 410], 16),
    (64, 16, 64, False, [300, 711, 410], 16),           # no centring: pad = 0, t = 0 is a frame's sample, the tail belongs to no frame
    (64, 16, 40, False, [300, 711, 410], 16),           # and win_length < n_fft: woff = 12 in the mel kernel
    (8192, 2048, 8192, True, [4200, 8292, 6200], 4),    # five frames: the tile's last frame and the next tile's first
    (8192, 4096, 8192, True, [4200, 12388, 8300], 1),   # four frames
]
MEL_KINDS = [("mel_power", {}), ("log_mel", {}), ("mel_db", dict(top_db=None)), ("mfcc", dict(top_db=None, n_mfcc=N_MFCC))]

# top_db: (kind, n_fft, hop, extra spec arguments, center); segment 1 is near-silent around a loud stretch (pcm_batch's burst)
TOP_DB = [0.0, 80.0, 20.0]
TOP_DB_SHAPES = [("mel_db", 64, 16, dict(n_mels=N_MELS), True), ("mfcc", 64, 16, dict(n_mels=N_MELS, n_mfcc=N_MFCC), True),
                 ("lin_db", 64, 16, {}, True), ("lin_db", 96, 24, {}, True), ("mel_db", 64, 16, dict(n_mels=N_MELS), False),
                 ("lin_db", 96, 24, {}, False)]
TOP_DB_IDS = ["%s_%d_%s" % (s[0], s[1], "c" if s[4] else "nc") for s in TOP_DB_SHAPES]
TOP_DB_LENGTHS, TOP_DB_BURST = [300, 900, 410], (500, 48)

# resampling: (r_in, r_out, lengths); 11025 -> 32000 (1280 / 441) is the pair whose table does not fit the LDS
RS_SHAPES = [(16000, 8000, [1500, 4500, 2100]), (8000, 16000, [1500, 4500, 2100]), (24000, 16000, [1500, 4500, 2100]),
             (11025, 32000, [900, 3100, 1300])]
RS_TILE, RS_TILES = 1024, 8  # outputs per tile of the resample kernel and tiles per workgroup (tests/test_nonfinite_cpu.py reads both
#                              in csrc/vsyn_resample.h, and the mel kernel's tiles and LDS image in csrc/vsyn_spectral.h)


def resample_positions(T, r_in, r_out):
    """t = 0, t = T - 1, an input whose outputs lie on both sides of an output tile's edge (and, where T_out reaches it, of a
    workgroup's), and a pair within one output's taps."""
    up, down = rm.ratio(r_in, r_out)
    To = rm.num_frames(r_in, r_out, T)
    pos = {"first": [0], "last": [T - 1]}
    for name, j in (("tile", RS_TILE), ("group", RS_TILES * RS_TILE)):
        if j + 1 < To:
            s = ((j - 1) * down + 10 * max(up, down)) // up  # i0 of output j - 1, its newest input: an older tap of output j
            fp = resample_footprint([s], T, r_in, r_out)
            assert fp[j - 1] and fp[j], (name, r_in, r_out)
            pos[name] = [s]
    pos["pair"] = [T // 3, T // 3 + 2]
    return pos


# PCEN: D = 5, segments of 3, 700 and 41 rows; the scan's blocks are 64 rows counted from a segment's first row ("PCEN", precision)
PCEN_D, PCEN_ROWS, PCEN_BLK, PCEN_COL = 5, [3, 700, 41], 64, 2
PCEN_DIRTY_ROWS = [0, PCEN_BLK - 1, PCEN_BLK, 699]
PCEN_KW = dict(sr=16000, hop_length=160)

# post stage: D = 5, orders 1 and 2, widths 3 and 9; segment 1 spans several workgroup tiles at every order
POST_D, POST_ROWS, POST_COL = 5, [12, 600, 41], 3
POST_ORDERS, POST_WIDTHS = (1, 2), (3, 9)


def post_dirty_rows(F, width):
    """An interior row, row h (the first interior row, which the h edge rows repeat), and the last interior row."""
    h = (width - 1) // 2
    return [F // 2 + 1, h, F - 1 - h]


def rows_batch(seg_rows, D, seed, positive):
    """(rows float32 [sum + 3][D], the segments' first rows): seeded rows back to back and three rows of NaN behind them. positive:
    a power spectrogram's spread (PCEN's input), else dB-like values."""
    rng = np.random.default_rng(seed)
    n = int(np.sum(seg_rows))
    x = 10.0 ** rng.uniform(-3.0, 3.0, (n, D)) if positive else rng.normal(-30.0, 12.0, (n, D))
    return np.concatenate([x.astype(np.float32), np.full((3, D), np.nan, np.float32)]), np.concatenate([[0], np.cumsum(seg_rows)])
