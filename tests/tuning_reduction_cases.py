"""The inputs of tests/test_gpu_tuning_reduction.py: the tuning stage (csrc/vsyn_tuning.h) on frames built to hold chosen peaks, shared
with tests/test_tuning_reduction_cpu.py, which asserts on the CPU, from the model alone (tests/tuning_model.py), that every crafted
peak is decided and that every case has the property it is there for. Everything comes from fixed seeds and phases.

The construction. With center=False and hop_length = win_length = n_fft the frames are disjoint, each its own signal. Under the
periodic Hann window a cosine of amplitude A exactly on bin k gives S[k] = A n / 4, S[k +- 1] = A n / 8 and rounding noise elsewhere,
which the threshold zeroes: k is the frame's only peak, its magnitude about A n / 4 (the interpolation's a is rounding noise), its
pitch k sr / n_fft, so that the segment's rate places the residual. Tones at least 3 bins apart do not interact. Tones on every other
bin with phases 0, pi, 0, pi, ... cancel on the bins between them: a band [k_lo, k_hi) of odd width with tones on k_lo, k_lo + 2, ...,
k_hi - 1 holds cap = (k_hi - k_lo + 1) / 2 peaks, the most a frame can need. Crafted peaks stay inside [2, NB - 3]: DC and Nyquist
collect the mirror image's leakage.

A LAUNCH is one spec (framing, power, tuning keywords) and its segments, which run in one call; a segment is dict(name, y float32 [T],
sr, frames (per frame the (k, A) of its tones, None for a segment that is no crafted one), claim). Claims, all checked on the model by
the CPU module and again on the device's own rows by the GPU module:
  klass       the byte (3: the top one .. 0) in which the order keys of the two middle magnitudes first differ; "equal" where every
              magnitude is identical. (Not claimed where n is odd and the values differ: both ranks are one element.)
  one_of      the name of a class that several candidate segments aim at (the two low bytes: rounding decides which byte splits);
              at least one candidate has to reach it.
  selected    the count of records at or above the median.
  tied        the number of histogram bins that share the largest count (the first wins); first_bin / last_bin: the winner is bin 0 /
              bin nbin - 1.
  at_cap      the fullest frame holds exactly cap records.

A. SELECT (n_fft 64 at 8000 Hz, band [2, 32)): tune_select2. n = 1, 2, 3, TUNE_WAVES - 1 .. TUNE_WAVES + 1 and 65 records of
   distinct magnitudes; two clusters of identical frames whose magnitudes (near 1.3 and 5.2; 1.25 and 1.75; a ratio of 1 + 2^-14;
   1 + 2^-20) split in the top byte, byte 2, byte 1 and byte 0, interleaved and (top byte) sorted descending; all frames identical, n
   even and odd; n = 9 with the median on five frames; 37 frames of three tones each (k, k + 4, k + 8), at power 1 and 2.
B. HIST (n_fft 64, the default band): the histogram's first arg-max. Two and three tones tie for the largest count (the frames of the
   lowest bin last; 2 g m - 1 records of which the g m tied ones are the upper half, so that the median selects exactly those whatever
   their last bits) at resolution 0.01, 0.3 (4 bins) and 1 / 4096 (the two bins more than 256 apart, in either order of their
   thread index b % 256; and, at another bins_per_octave, a multiple of 256 apart: one thread's stride); the winner in bin 0 and in
   bin nbin - 1 (k = 5 at rates found by search, residuals within 1e-4 of -0.5 and +0.5), two segments at two rates; one record.
C. CAP: pip_rows' compaction at exactly cap records a frame: n_fft 512 in the default band (45), in [2, 255) (127: two lane strides
   of tune_each, every 64-bin group of pip_rows and the last group of one lane), n_fft 64 in [3, 30) (14); such frames first, in the
   middle and last of a tile beside sparse and silent frames, frame counts tile - 1, tile, tile + 1.
D. TILE1: vsyn_piptrack_direct_kernel<1>, (n_fft, hop) = (4410, 1102) centred and (8190, 2047) not centred, 1, 2 and 3 frames of
   tuning_model.chord at power 1 and 2 (natural input: no claim but that there are peaks).
E. EMPTY: a crafted segment, one of 63 samples (no frame), a silent one, one whose only tone lies outside the band, a crafted one.
"""
import functools

import numpy as np

from tests import spectral_lin_model as lm
from tests import tuning_model as tm

TUNE_WAVES = 4  # csrc/vsyn_tuning.h
SR_A = 8000     # n_fft 64: bins of 125 Hz, the default band is [2, 32)
SR = 22050


def frame(n_fft, tones, alternate=False):
    """One frame: the sum of A cos(2 pi k t / n_fft + phase) over tones [(k, A)]; phase 0, or 0, pi, 0, ... in the order given."""
    t = np.arange(n_fft, dtype=np.float64)
    y = np.zeros(n_fft)
    for i, (k, A) in enumerate(tones):
        y += A * np.cos(2.0 * np.pi * k * t / n_fft + (np.pi * (i & 1) if alternate else 0.0))
    return y.astype(np.float32)


def seg(name, n_fft, sr, frames, claim=None, alternate=False):
    y = np.concatenate([frame(n_fft, f, alternate) for f in frames]) if frames else np.zeros(0, np.float32)
    return dict(name=name, y=y, sr=sr, frames=frames, claim=dict(claim or {}))


def launch(name, n_fft, segs, power=1, tun=None, hop=None, center=False):
    return dict(name=name, n_fft=n_fft, hop=n_fft if hop is None else hop, win=n_fft, center=center, power=power, tun=dict(tun or {}), segs=segs)


def params(L):
    """The model's keywords of a launch: fmin, fmax, threshold, resolution, bins_per_octave."""
    return dict(tm.DEFAULTS, **L["tun"])


# ---- what the claims are read from: shared by the CPU module (model rows) and the GPU module (the device's rows) ----

def key(x):
    """The order key of float32 x (csrc/vsyn_spectral.h, spec_key)."""
    b = int(np.float32(x).view(np.uint32))
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def split_byte(a, b):
    """The byte (3 .. 0) in which the keys of a and b first differ from the top; None when they are equal."""
    x = key(a) ^ key(b)
    return None if x == 0 else (x.bit_length() - 1) // 8


def klass(pitch, mag):
    """The selection's regime on rows: "none" (no record), "equal" (all magnitudes identical), "odd" (one middle element), "tie" (the
    two middle elements equal, others differ), or the byte in which the two middle keys split."""
    m = np.sort(mag[pitch > 0])
    n = m.size
    if n == 0:
        return "none"
    if m[0] == m[-1]:
        return "equal"
    if n & 1:
        return "odd"
    s = split_byte(m[(n - 1) // 2], m[n // 2])
    return "tie" if s is None else s


def histogram(pitch, mag, resolution, bins_per_octave):
    """(counts [nbin], margin): the selected records' histogram as tuning_model.pitch_tuning counts it, and the least distance of a
    selected residual from any edge."""
    keep = pitch > 0
    p, m = pitch[keep], mag[keep]
    e = tm.edges(resolution)
    if p.size == 0:
        return np.zeros(e.size - 1, np.int64), np.inf
    p = p[m >= np.median(m)]
    r = tm.residuals(p, bins_per_octave)
    idx = np.searchsorted(e, r, side="right") - 1
    return np.bincount(idx, minlength=e.size - 1), float(np.abs(r[:, None] - e[None, :]).min())


def winners(counts):
    """The bins that share the largest count."""
    return [] if counts.max() == 0 else np.nonzero(counts == counts.max())[0].tolist()


def per_frame(pitch):
    return (pitch > 0).sum(axis=1)


def cap(L, sr):
    p = params(L)
    k_lo, k_hi = tm.bins(sr, L["n_fft"], p["fmin"], p["fmax"])
    return (k_hi - k_lo + 1) // 2


# ---- A ----

def _amps(n, seed, lo=0.05, hi=0.15):
    a = np.random.default_rng(seed).uniform(lo, hi, n)
    assert np.unique(a.astype(np.float32)).size == n
    return a.tolist()


def _clusters(name, lo, hi, order, claim):
    """order: a string of L and H, one frame each, k = 5."""
    return seg(name, 64, SR_A, [[(5, lo if c == "L" else hi)] for c in order], claim)


LOW_BASES = (0.07, 0.083, 0.091, 0.11)


def select_segments():
    segs = []
    for n in (1, 2, 3, TUNE_WAVES - 1, TUNE_WAVES, TUNE_WAVES + 1, 65):
        segs.append(seg("n%d" % n, 64, SR_A, [[(5, A)] for A in _amps(n, 100 + n)], dict(n=n)))
    # S[k] = 16 A at n_fft 64
    segs.append(_clusters("top", 1.3 / 16, 5.2 / 16, "LHHLHLLHLH", dict(klass=3, selected=5)))
    segs.append(_clusters("top_desc", 1.3 / 16, 5.2 / 16, "HHHHHLLLLL", dict(klass=3, selected=5)))
    segs.append(_clusters("byte2", 1.25 / 16, 1.75 / 16, "HLLHLHHLHLLH", dict(klass=2, selected=6)))
    for i, base in enumerate(LOW_BASES):
        segs.append(_clusters("byte1_%d" % i, base, base * (1.0 + 2.0 ** -14), "LHLHHL", dict(one_of=1, selected=3)))
        segs.append(_clusters("byte0_%d" % i, base, base * (1.0 + 2.0 ** -20), "HLHLLHLH", dict(one_of=0, selected=4)))
    segs.append(_clusters("same_even", 0.1, 0.1, "L" * 8, dict(klass="equal", selected=8)))
    segs.append(_clusters("same_odd", 0.1, 0.1, "L" * 7, dict(klass="equal", selected=7)))
    lo, mid, hi = 0.06, 0.09, 0.13
    segs.append(seg("median_tie", 64, SR_A, [[(5, A)] for A in (mid, hi, lo, mid, mid, lo, mid, hi, mid)], dict(klass="odd", selected=7)))
    return segs


def multi_segment():
    rng = np.random.default_rng(7)
    frames = []
    for f in range(37):
        k = 3 + int(rng.integers(0, 4))
        a = rng.uniform(0.08, 0.2, 3)  # within a factor 2.5: at power 2 the smallest is 0.16 of the largest, above the threshold 0.1
        frames.append([(k, float(a[0])), (k + 4, float(a[1])), (k + 8, float(a[2]))])
    return seg("three_tones", 64, SR_A, frames, dict(n=111))


# ---- B ----

@functools.lru_cache(maxsize=None)
def find_rate(ks, resolution, bpo=12, rule="distinct", near=None):
    """The first rate in 8000 .. 48000 at which every tone of ks (n_fft 64) lies in the default band and inside [2, 30], every
    residual of the exact bin frequency (rounded to float32, as the pitch is) keeps 2e-5 from every edge, and the rule holds for
    the tones' bins (all but the last of ks, which is the filler's). near: the residual of ks[0] lies within 1e-4 of it instead."""
    sr = np.arange(8000, 48001)
    ok = np.ones(sr.size, bool)
    e = tm.edges(resolution)
    idx = []
    for k in ks:
        f = k * sr / 64.0
        ok &= (f >= 150.0) & (f < np.minimum(4000.0, sr / 2.0)) & (2 <= k <= 30)
        r = tm.residuals(f.astype(np.float32), bpo)
        ok &= np.abs(r[:, None] - e[None, :]).min(axis=1) >= 2e-5
        if near is not None:
            ok &= np.abs(r - near) < 1e-4
        idx.append(np.searchsorted(e, r, side="right") - 1)
    b = np.array(idx[:-1] if len(ks) > 1 else idx)
    if rule == "distinct":
        for i in range(len(b)):
            for j in range(i):
                ok &= b[i] != b[j]
    else:
        lo, hi = b.min(axis=0), b.max(axis=0)
        ok &= hi - lo > 256
        if rule == "far":          # the first bin's thread is the lower one
            ok &= lo % 256 < hi % 256
        elif rule == "far_swapped":  # the first bin's thread is the higher one
            ok &= lo % 256 > hi % 256
        elif rule == "same_thread":  # one thread meets both, the first bin first
            ok &= (hi - lo) % 256 == 0
    hit = np.nonzero(ok)[0]
    return int(sr[hit[0]]) if hit.size else None


@functools.lru_cache(maxsize=None)
def same_thread_bpo():
    """(bins_per_octave, (k1, k2)): the first pair whose bins at resolution 1 / 4096 can lie a multiple of 256 apart."""
    for bpo in range(1, 257):
        for ks in ((4, 5), (3, 5), (3, 4), (4, 7), (5, 7)):
            d = (bpo * np.log2(ks[1] / ks[0])) % 1.0 * 16.0
            if 0.5 < d < 15.5 and abs(d - round(d)) < 0.3 / 256.0 and find_rate(ks + (3 if 3 not in ks else 6,), 1.0 / 4096.0, bpo, "same_thread"):
                return bpo, ks
    raise AssertionError("no pair found")


def tie_segment(name, ks, sr, resolution, bpo=12, m=4, A=0.1):
    """g = len(ks) - 1 tones on m frames each at amplitude A and 2 g m - 1 records in all: the g m - 1 filler frames (ks[-1], A / 4)
    are the lower half, the median is the smallest tied record, and exactly the tied ones are selected. The frames of the tone in
    the lowest bin come last."""
    tones, filler = list(ks[:-1]), ks[-1]
    r = tm.residuals(np.array([k * sr / 64.0 for k in tones], np.float32), bpo)
    tones = [k for _, k in sorted(zip(r.tolist(), tones), reverse=True)]  # by residual, descending: the first bin's frames last
    g = len(tones)
    frames, fill = [], g * m - 1
    for k in tones:
        for _ in range(m):
            frames.append([(k, A)])
            if fill:
                frames.append([(filler, A / 4.0)])
                fill -= 1
    return seg(name, 64, sr, frames, dict(tied=g, selected=g * m, n=2 * g * m - 1))


def edge_segments():
    lo = find_rate((5,), 0.01, near=-0.5)
    hi = find_rate((5,), 0.01, near=0.5)
    return [seg("first_bin", 64, lo, [[(5, 0.1)]] * 3, dict(first_bin=True, selected=3)),
            seg("last_bin", 64, hi, [[(5, 0.1)]] * 3, dict(last_bin=True, selected=3))]


def hist_launches():
    out = []
    one = seg("one_record", 64, 11025, [[(5, 0.1)]], dict(n=1, selected=1, tied=1))
    r = 0.01
    out.append(launch("hist_0.01", 64, [tie_segment("tie2", (4, 5, 3), find_rate((4, 5, 3), r), r),
                                         tie_segment("tie3", (4, 5, 7, 3), find_rate((4, 5, 7, 3), r), r, m=3)] + edge_segments() + [one], tun=dict(resolution=r)))
    r = 0.3
    out.append(launch("hist_0.3", 64, [tie_segment("tie2", (4, 5, 3), find_rate((4, 5, 3), r), r),
                                        tie_segment("tie3", (4, 5, 7, 3), find_rate((4, 5, 7, 3), r), r, m=3)] + edge_segments() + [one], tun=dict(resolution=r)))
    r = 1.0 / 4096.0
    out.append(launch("hist_4096_bins", 64, [tie_segment("far", (4, 5, 3), find_rate((4, 5, 3), r, rule="far"), r),
                                           tie_segment("far_swapped", (4, 5, 3), find_rate((4, 5, 3), r, rule="far_swapped"), r),
                                           tie_segment("tie3", (4, 5, 7, 3), find_rate((4, 5, 7, 3), r), r, m=3)] + edge_segments() + [one],
                      tun=dict(resolution=r)))
    bpo, ks = same_thread_bpo()
    ks = ks + (3 if 3 not in ks else 6,)
    out.append(launch("hist_same_thread", 64, [tie_segment("same_thread", ks, find_rate(ks, r, bpo, "same_thread"), r, bpo)],
                      tun=dict(resolution=r, bins_per_octave=bpo)))
    return out


# ---- C ----

def cap_segments(n_fft, L_tun, tile, A):
    p = dict(tm.DEFAULTS, **L_tun)
    k_lo, k_hi = tm.bins(SR, n_fft, p["fmin"], p["fmax"])
    assert (k_hi - k_lo) % 2 == 1 and k_lo >= 2 and k_hi <= n_fft // 2 - 1
    dense = [(k, A) for k in range(k_lo, k_hi, 2)]
    sparse = [(k_lo + 4, 3.0 * A)]
    rest = [sparse, []]

    def seg_of(name, F, at):
        frames = [dense if f in at else rest[(f + len(at)) % 2] for f in range(F)]
        return seg(name, n_fft, SR, frames, dict(at_cap=True), alternate=True)
    return [seg_of("first_Tm1", tile - 1, (0,)), seg_of("last_T", tile, (tile - 1,)), seg_of("middle_and_next_Tp1", tile + 1, (tile // 2, tile)),
            seg_of("all_dense", 2, (0, 1)), seg_of("sparse_only", tile, ())]


def band(n_fft, k_lo, k_hi):
    """fmin, fmax that give the band [k_lo, k_hi) at SR."""
    hz = SR / n_fft
    return dict(fmin=(k_lo - 0.5) * hz, fmax=(k_hi - 0.5) * hz)


def cap_launches():
    wide, small = band(512, 2, 255), band(64, 3, 30)
    out = [launch("cap_512_default", 512, cap_segments(512, {}, 4, 0.01)),
           launch("cap_512_wide", 512, cap_segments(512, wide, 4, 0.01), tun=wide),
           launch("cap_512_wide_p2", 512, cap_segments(512, wide, 4, 0.01), power=2, tun=wide),
           launch("cap_64", 64, cap_segments(64, small, 32, 0.02), tun=small)]
    for L in out:
        L["segs"][-1]["claim"] = {}  # the sparse segment stands beside the dense ones: no frame at cap
    return out


# ---- D ----

TILE1 = [(4410, 1102, True), (8190, 2047, False)]


def tile1_launches():
    out = []
    for n, hop, center in TILE1:
        # the longest signals of 1, 2 and 3 frames
        segs = [dict(name="chord_%d" % F, y=tm.chord(F * hop - 1 + (0 if center else n), SR, tm.GRID_DETUNE, seed=F), sr=SR, frames=None,
                     claim=dict(F=F)) for F in (1, 2, 3)]
        for power in (1, 2):
            out.append(launch("tile1_%d_p%d" % (n, power), n, segs, power=power, hop=hop, center=center))
    return out


# ---- E ----

def empty_launch():
    short = dict(name="no_frame", y=frame(64, [(5, 0.1)])[:63], sr=SR, frames=[], claim=dict(n=0, F=0))
    return launch("empty", 64, [seg("crafted_a", 64, SR, [[(5, A)] for A in _amps(5, 31)], dict(n=5)),
                                short,
                                seg("silent", 64, SR, [[], [], []], dict(n=0, F=3)),
                                seg("out_of_band", 64, SR, [[(20, 0.1)], [(24, 0.2)]], dict(n=0, F=2)),
                                seg("crafted_b", 64, SR, [[(7, A)] for A in _amps(4, 32)], dict(n=4))])


@functools.lru_cache(maxsize=None)
def launches():
    """group -> list of launches."""
    return dict(select=[launch("select_p1", 64, select_segments() + [multi_segment()]), launch("select_p2", 64, [multi_segment()], power=2)],
                hist=hist_launches(), cap=cap_launches(), tile1=tile1_launches(), empty=[empty_launch()])


def model_rows(L, s):
    """(S, dS, pitch, mag) of a segment from the model alone: the float64 spectrum with its bound, and piptrack on its float32 rounding."""
    p = params(L)
    X, B = lm.stft(s["y"], L["n_fft"], L["hop"], L["win"], L["center"])
    S, dS = lm.power_bound(X, B, L["power"])
    pitch, mag = tm.piptrack(S.astype(np.float32), s["sr"], L["n_fft"], p["fmin"], p["fmax"], p["threshold"])
    return S, dS, pitch, mag
