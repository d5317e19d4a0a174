"""Float64 model of the beat tracker (include/vorbis_synth_hip.h, rhythm section D: librosa >= 0.10.2's static-tempo __beat_tracker,
restated), with the error bounds and decision bands the GPU tests gate on. numpy only, in literal loops (a loop over the window's k,
over the frames of the dynamic programme, over the beats); tests/test_beat_cpu.py checks it against a vectorised restatement in
numpy's and scipy's own words.

What two correct evaluations of section D can differ in, e = 2^-53:
  tables           w[k] = exp(..) and tx[d] = -tightness (log d - log P)^2 come from two maths libraries (the library's host code, numpy
                   here). exp and log are within one ulp of the exact value in both, so w differs by at most 2 e |w|, log d - log P by
                   2 e (|log d| + |log P|) + e |difference|, and tx[d] by TXE[d] = tightness (2 |q| (2 e (|log d| + |log P|) + e |q|)
                   + 3 e q^2), q = log d - log P: the error of q doubled by the square, the square's and the product's roundings.
                   tx[P] = 0 in both (the same number is subtracted from itself).
  sd               the model adds in the device's documented order (ordered_sum) and the device writes no fma there, so m and the sum
                   of squares agree bit for bit unless a division or the square root is not correctly rounded: sd within SD_REL = 4 e
                   of the model's, relatively, and exactly equal when the model's is 0 (every x[n] - m is then an exact 0 in any
                   evaluation that gets the same m). u inherits that: |du| <= SD_REL |u|.
  ls               the device's fma chain against the model's multiply-and-add chain over the same k, n = terms of the frame: either
                   is within n e A[i] of the exact sum, A[i] = sum_k |w[k] u[i - k]|, so LSB[i] = (2 n e + 2 e + SD_REL) A[i]
                   (the chains, the tables, sd). A[i] = 0 (a stretch of zeros wider than the window) gives LSB[i] = 0: every
                   product is an exact 0 in any evaluation.
  cum              propagated along the chain, a frame's bound being its own, the largest in its window and two roundings: CB[i] = LSB[i] + max over the candidates' CB[loc] + TXE of the
                   chosen d + e |s_best| + e |cum[i]| (the two additions). No candidate: CB[i] = LSB[i].
  decisions        each comparison below has a margin (how far apart the two sides are here) and a band (how far two correct
                   evaluations of that difference can be apart). It is decided when margin > band, or when band = 0 (both sides are
                   exact in every evaluation, so equal values are equal everywhere and the stated tie rule applies):
    arg-max at i     margin s_best - s_second (0 on a tie), band 2 (max CB over the candidates + max TXE over them + e |s_best|);
    i0               for i <= i0: margin |ls[i] - thr|, band LSB[i] + 0.01 max LSB + 2 e |thr|;
    local maximum    for every i and either neighbour j: margin |cum[i] - cum[j]|, band CB[i] + CB[j]; band 0 where the later of
                     the two is the earlier one with nothing added (P = 1, d = 1 chosen by a decided arg-max, so tx[1] = 0, and
                     |ls| + LSB at most e / 4 of it, half of what rounding to nearest absorbs): a plateau of cum, equal in every
                     evaluation, which the > and >= of the rule then decide;
    tail             for every local maximum i from the tail upwards: margin |cum[i] - 0.5 med|, band CB[i] + 0.5 max CB over the
                     local maxima + 2 e |med| (the median is one of them, or the mean of two);
    trim             t is within TB = 2 max LSB over the beats + (B + 8) e t of any other evaluation (sm is v[j-1]/2 + v[j] + v[j+1]/2,
                     at most 2 max LSB off; the root mean square of values off by d is off by at most d; B + 8 roundings); for
                     i <= n0 and i >= n1: margin |ls[i] - t|, band LSB[i] + TB.
  beat_track()'s "worst" is the smallest margin / band over all of them (Inf where every band is 0); "smallest_rel" is the smallest
  arg-max margin relative to |s_best|.
Given decided comparisons the integers (i0, back, the local maxima, tail, beats, counts) are the same in every evaluation, and the
device's ls and cum lie within LSB and CB of the model's."""
import numpy as np

E64 = 2.0 ** -53
FLT_MIN = float(np.finfo(np.float32).tiny)
MAX_PERIOD = 2048
SD_REL = 4 * E64


def rint(v):
    """Half to even, as C's rint in the default rounding mode."""
    return int(np.rint(v))


def period(bpm, rate, hop):
    """Step D.0: P, or 0 for a period outside [1, 2048] (refusal word 3)."""
    v = np.rint(60.0 * (float(rate) / float(hop)) / float(bpm))
    return int(v) if 1 <= v <= MAX_PERIOD else 0


def ordered_sum(v):
    """The order of D.1's two sums: 256 partials, partial t adding its terms n = t, t + 256, .. in that order to 0.0; in each group of
    64 consecutive partials six rounds o = 32 .. 1 in which partial i becomes partial i + partial (i xor o); then the four groups'
    sums added in ascending order to 0.0."""
    v = np.asarray(v, np.float64)
    part = np.zeros(256)
    for r in range(0, len(v), 256):
        blk = v[r:r + 256]
        part[:len(blk)] = part[:len(blk)] + blk
    part = part.reshape(4, 64)
    lanes = np.arange(64)
    o = 32
    while o >= 1:
        part = part + part[:, lanes ^ o]
        o >>= 1
    s = 0.0
    for g in range(4):
        s = s + float(part[g, 0])
    return s


def normalise(x):
    """Step D.1: (u, sd). F >= 2."""
    x = np.asarray(x, np.float32).astype(np.float64)
    F = len(x)
    m = ordered_sum(x) / F
    d = x - m
    sd = float(np.sqrt(ordered_sum(d * d) / (F - 1)))
    return x / (sd + FLT_MIN), sd


def window(P):
    """w[k + P], k = -P .. P."""
    k = np.arange(-P, P + 1, dtype=np.float64)
    return np.exp(-0.5 * (32.0 * k / P) ** 2)


def local_score(u, P):
    """Step D.2: (ls, A, n): the chain with k ascending, sum |w u|, and the terms of each frame."""
    F = len(u)
    w = window(P)
    ls, A, n = np.zeros(F), np.zeros(F), np.zeros(F)
    for k in range(-P, P + 1):  # i - k in [0, F)
        a, b = max(0, k), min(F, F + k)
        if a >= b:
            continue
        t = w[k + P] * u[a - k:b - k]
        ls[a:b] = ls[a:b] + t
        A[a:b] = A[a:b] + np.abs(t)
        n[a:b] += 1
    return ls, A, n


def half(P):
    """(h, lo) of D.3."""
    h = rint(P / 2.0)
    return h, max(h, 1)


def transition(P, tightness):
    """(tx, TXE) indexed by d, d in [lo, 2P] (entries below lo unused)."""
    lo = half(P)[1]
    d = np.arange(0, 2 * P + 1, dtype=np.float64)
    d[:lo] = lo
    q = np.log(d) - np.log(float(P))
    tx = -float(tightness) * q ** 2
    txe = float(tightness) * (2 * np.abs(q) * (2 * E64 * (np.abs(np.log(d)) + abs(np.log(float(P)))) + E64 * np.abs(q)) + 3 * E64 * q ** 2)
    return tx, txe


def beat_track(x, P, tightness=100.0, trim=True):
    """Steps D.1 to D.5 on a float32 envelope and a period P >= 1. Returns a dict: refused (1 for a non-finite envelope, else 0), beats
    (int64), ls, cum, back (int32, F entries each; empty for a segment without a score), LSB, CB, i0, tail, maxima (the local maxima's count), worst, worst_at,
    smallest_rel, scored."""
    x = np.asarray(x, np.float32)
    F = len(x)
    none = dict(refused=0, beats=np.zeros(0, np.int64), ls=np.zeros(0), cum=np.zeros(0), back=np.zeros(0, np.int32), LSB=np.zeros(0),
                CB=np.zeros(0), i0=0, tail=-1, worst=np.inf, worst_at="", smallest_rel=np.inf, scored=False, maxima=0)
    if not np.all(np.isfinite(x)):
        return dict(none, refused=1)
    if F < 2 or not np.any(x != 0):
        return none
    worst = [np.inf, ""]

    def decide(margin, band, what="", i=0):
        if band > 0 and margin / band < worst[0]:
            worst[:] = [margin / band, "%s at frame %d: margin %.3g, band %.3g" % (what, i, margin, band)]

    u, sd = normalise(x)
    ls, A, n = local_score(u, P)
    LSB = (2 * n * E64 + 2 * E64 + (SD_REL if sd > 0 else 0.0)) * A
    thr = 0.01 * float(ls.max())
    reach = ls >= thr
    i0 = int(np.argmax(reach)) if reach.any() else F  # (a negative maximum: no frame reaches thr, every back is -1)
    for i in range(min(i0 + 1, F)):
        decide(abs(ls[i] - thr), LSB[i] + 0.01 * LSB.max() + 2 * E64 * abs(thr), "i0", i)
    # the dynamic programme
    lo = half(P)[1]
    tx, TXE = transition(P, tightness)
    cum, CB, back = np.zeros(F), np.zeros(F), np.full(F, -1, np.int32)
    same = np.zeros(F, bool)  # cum[i] is cum[i - 1] in every evaluation (P = 1): tx[1] = 0 and an ls[i] far below half an ulp added to it
    smallest_rel = np.inf
    for i in range(F):
        hi = min(2 * P, i)
        if hi < lo:
            cum[i], CB[i] = ls[i], LSB[i]
            continue
        s = cum[i - hi:i - lo + 1][::-1] + tx[lo:hi + 1]  # d ascending
        k = int(np.argmax(s))  # the largest s; the first of them, which is the smallest d, on a tie
        best_s, best_d = float(s[k]), lo + k
        s[k] = -np.inf
        second = float(s.max())
        cbw = float(CB[i - hi:i - lo + 1].max())
        if hi > lo:
            decide(best_s - second, 2 * (cbw + float(TXE[lo:hi + 1].max()) + E64 * abs(best_s)), "arg-max", i)
            if best_s != 0:
                smallest_rel = min(smallest_rel, (best_s - second) / abs(best_s))
        cum[i] = ls[i] + best_s
        CB[i] = LSB[i] + cbw + TXE[best_d] + E64 * abs(best_s) + E64 * abs(cum[i])
        same[i] = best_d == 1 and P == 1 and abs(ls[i]) + LSB[i] <= 0.25 * E64 * abs(best_s)
        if i >= i0:
            back[i] = i - best_d
    # the last beat
    ismax = np.zeros(F, bool)
    for i in range(F):
        a, b = max(i - 1, 0), min(i + 1, F - 1)
        ismax[i] = cum[i] > cum[a] and cum[i] >= cum[b]
        for j in (a, b):
            if j != i and not same[max(i, j)]:
                decide(abs(cum[i] - cum[j]), CB[i] + CB[j], "local maximum", i)
    idx = np.flatnonzero(ismax)
    out = dict(refused=0, ls=ls, cum=cum, back=back, LSB=LSB, CB=CB, i0=i0, tail=-1, scored=True, smallest_rel=smallest_rel, maxima=len(idx), u=u, sd=sd)
    if len(idx) == 0:
        return dict(out, beats=np.zeros(0, np.int64), worst=worst[0], worst_at=worst[1])
    srt = np.sort(cum[idx])
    M = len(srt)
    med = float(srt[M // 2]) if M % 2 else float((srt[M // 2 - 1] + srt[M // 2]) / 2.0)
    tail = F - 1
    for i in idx[::-1]:
        decide(abs(cum[i] - 0.5 * med), CB[i] + 0.5 * float(CB[idx].max()) + 2 * E64 * abs(med), "tail", i)
        if cum[i] >= 0.5 * med:
            tail = int(i)
            break
    beats = []
    b = tail
    while b >= 0:
        beats.append(b)
        b = int(back[b])
    beats = np.array(beats[::-1], np.int64)
    out["tail"] = tail
    # the trim
    B = len(beats)
    v = ls[beats]
    t = 0.0
    if trim:
        acc = 0.0
        for j in range(B):
            sm = (0.5 * v[j - 1] if j > 0 else 0.0) + v[j] + (0.5 * v[j + 1] if j + 1 < B else 0.0)
            acc = acc + sm * sm
        t = 0.5 * float(np.sqrt(acc / B))
    TB = 2 * float(LSB[beats].max()) + (B + 8) * E64 * t if trim else 0.0
    over = np.flatnonzero(ls > t)
    if len(over) == 0:
        for i in range(F):
            decide(abs(ls[i] - t), LSB[i] + TB, "trim", i)
        return dict(out, beats=np.zeros(0, np.int64), worst=worst[0], worst_at=worst[1])
    n0, n1 = int(over[0]), int(over[-1])
    for i in list(range(n0 + 1)) + list(range(n1, F)):
        decide(abs(ls[i] - t), LSB[i] + TB, "trim", i)
    return dict(out, beats=beats[(beats >= n0) & (beats <= n1)], worst=worst[0], worst_at=worst[1])
