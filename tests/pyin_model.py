"""The float64 model of the pyin stage (include/vorbis_synth_hip.h, "pyin"), written out step by step in numpy. It is the contract
the device is compared against; tests/test_pyin_cpu.py compares it against a restatement in librosa's own words. Steps 1 to 5 of
"pitch" come from tests/pitch_model.py.

Besides the values the model returns, for EVERY discrete decision, a margin and the band inside which two correct float64
evaluations (this model and the device) may disagree; a case counts as decided when every margin is above its band. The bands are
derived here, from pitch_model.band, the lengths of the chains and a propagated bound on the Viterbi's values; none is tuned on the
device. Band 0 holds where both sides evaluate the same expression of the same bits (an exact frame, two exact zeros, equal table
entries added to equal values): there the lower index wins on both sides.

    h_k < t_m, the troughs themselves, the arg-min g: relative gaps of c against pitch_model.band.
    P_k > 0: P_k is a sum of non-negative terms that depends on c through decisions only: decided when it is 0 by structure or at
             least 1e-300 (far from the subnormal range, where exp may round differently).
    rint of the bin and the clip at B: the distance of x = 12 bps log2(f0 / fmin) from the nearest half integer, against the error
             of x from pitch_model.f0_tolerance (the parabolic shift) and the roundings of the division and the logarithm.
    back pointers on the optimal path and the final arg-max: the gap in log units between the best and the next source, against
             twice the propagated bound E[t] on |value(device) - value(model)|.
"""
import math

import numpy as np

from tests import pitch_model as pm

TINY = pm.TINY
U = pm.U
LT = math.log(TINY)
P_FLOOR = 1e-300


def thresholds(N):
    """Step 3: t_m = m * (1 / N), m < N, and t_N = 1."""
    t = np.arange(1, N + 1, dtype=np.float64) * (1.0 / N)
    t[-1] = 1.0
    return t


def num_bins(fmin, fmax, resolution):
    """(bps, B) of step 5."""
    bps = int(math.ceil(1.0 / resolution))
    return bps, int(math.floor(12 * bps * math.log2(float(fmax) / float(fmin)))) + 1


def width(sr, H, max_transition_rate, bps):
    """w of step 6 (Python's round: half even)."""
    return int(round(max_transition_rate * 12 * H / sr)) * bps + 1


def triangle(w):
    """scipy.signal.get_window("triangle", w, fftbins=False) for odd w."""
    k = np.arange(w, dtype=np.float64)
    return ((w + 1) / 2.0 - np.abs(k - w // 2)) / ((w + 1) / 2.0)


def loc_formula(B, w):
    """Step 6 by its formula: (B, B), every row divided by its sum."""
    h = w // 2
    i = np.arange(B)
    dist = np.abs(i[None, :] - i[:, None])
    loc = np.where(dist <= h, ((w + 1) / 2.0 - dist) / ((w + 1) / 2.0), 0.0)
    return loc / loc.sum(axis=1, keepdims=True)


def loc_librosa(B, w):
    """Step 6 by librosa.sequence.transition_local's own route (pad_center, roll, truncate), which needs w <= B."""
    win = triangle(w)
    lpad = (B - w) // 2
    out = np.zeros((B, B))
    for i in range(B):
        row = np.roll(np.pad(win, (lpad, B - w - lpad)), B // 2 + i + 1)
        row[min(B, i + w // 2 + 1):] = 0
        row[:max(0, i - w // 2)] = 0
        out[i] = row
    return out / out.sum(axis=1, keepdims=True)


def loc_matrix(B, w):
    assert w % 2 == 1
    return loc_librosa(B, w) if w <= B else loc_formula(B, w)


def log_transition(B, w, switch_prob):
    """log(kron([[1 - s, s], [s, 1 - s]], loc) + tiny): (2B, 2B), [source][target]."""
    s = float(switch_prob)
    return np.log(np.kron(np.array([[1.0 - s, s], [s, 1.0 - s]]), loc_matrix(B, w)) + TINY)


def band_table(lt, B, w):
    """The (B, w, 2) layout of vsyn_pyin_transition from the dense log table: [i][j - i + h][same, other voicing]; log(tiny) where j
    is outside [0, B)."""
    h = w // 2
    out = np.full((B, w, 2), LT)
    for i in range(B):
        for k in range(w):
            j = i + k - h
            if 0 <= j < B:
                out[i, k, 0] = lt[i, j]
                out[i, k, 1] = lt[i, B + j]
    return out


def trough_mask(c):
    n = c.shape[0]
    tr = np.zeros(n, bool)
    tr[1:-1] = (c[1:-1] < c[:-2]) & (c[1:-1] <= c[2:])
    tr[0] = c[0] < c[1]
    tr[-1] = c[-1] < c[-2]
    return tr


def shift_of(c, i):
    """Step 7 of "pitch" at index i: dict(i, a, b, shift)."""
    a = b = shift = 0.0
    if 0 < i < c.shape[0] - 1:
        a = (c[i + 1] + c[i - 1]) - 2.0 * c[i]
        b = (c[i + 1] - c[i - 1]) / 2.0
        if abs(b) < abs(a):
            shift = -b / a
    return dict(i=i, a=float(a), b=float(b), shift=float(shift))


def p_bound(N, K, lam):
    """The relative distance of two float64 evaluations of P_k (given the same decisions): a chain of N additions of non-negative
    terms (N U); per term the product of three factors (2 U), the quotient of 1 - e^-lam and 1 - e^(-lam n) (for lam >= 0.5 both
    differences are at least 0.39 of quantities below 1 that an exp of at most 2 ulp gives: 10 U in all), and e^(-lam pos), whose
    argument rounds by |lam pos| U and whose value by 2 ulp; the no-trough term adds a chain of N and two roundings. Twice, for two
    evaluations."""
    assert lam >= 0.5
    return 2 * (2 * N + 2 * lam * K + 20) * U


def frame_observation(c, sr, p_min, fmin, bps, B, thr, beta, lam, ntp, band, exact, L, p_max):
    """Steps 2 to 5 for one frame's c: dict(lags, h, P, bins, x, obs (B,), vp, margins: a list of (name, margin, band))."""
    n = c.shape[0]
    N = thr.shape[0]
    marg = []
    cband = 0.0 if exact else band
    tr = trough_mask(c)
    if not exact:
        marg.append(("trough", float(pm._gap(c[1:], c[:-1]).min()), cband))
    lags = np.flatnonzero(tr)
    K = lags.size
    obs = np.zeros(B)
    out = dict(lags=lags, h=c[lags], P=np.zeros(K), bins=np.full(K, -1, np.int64), x=np.zeros(K), obs=obs, vp=0.0, margins=marg, pbound=p_bound(N, max(K, 1), lam))
    if K == 0:
        return out
    h = c[lags]
    below = np.less.outer(h, thr)  # (K, N)
    if not exact:
        g_ht = pm._gap(h[:, None], thr[None, :])
        g_ht = np.where(h[:, None] == 0.0, np.inf, g_ht)  # an exact zero is below every threshold on both sides
        marg.append(("below", float(g_ht.min()), cband))
    n_m = below.sum(axis=0)
    pos = np.cumsum(below, axis=0) - 1
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        fact = (1.0 - np.exp(-lam)) / (1.0 - np.exp(-lam * n_m.astype(np.float64)))
        prior = fact[None, :] * np.exp(-lam * pos.astype(np.float64))
        terms = np.where(below, prior * beta[None, :], 0.0)
    P = np.cumsum(terms, axis=1)[:, -1]  # one chain, m ascending
    g = int(np.argmin(h))
    if K > 1 and not exact:
        others = np.delete(h, g)
        gap = pm._gap(np.full(K - 1, h[g]), others)
        gap = np.where((others == 0.0) & (h[g] == 0.0), np.inf, gap)  # two exact zeros: the first wins on both sides
        marg.append(("argmin", float(gap.min()), cband))
    rest = np.where(~below[g], beta, 0.0)
    P[g] += ntp * (np.cumsum(rest)[-1] if N else 0.0)
    structural_zero = ~(below & (beta[None, :] > 0.0)).any(axis=1)  # every term is a product with an exact 0 (underflow is not structural)
    structural_zero[g] = structural_zero[g] and (ntp == 0.0 or not (rest > 0).any())
    pos_margin = np.where(P > 0, P, np.where(structural_zero, np.inf, 0.0))
    marg.append(("P>0", float(pos_margin.min()), P_FLOOR))
    out["P"] = P
    if (n_m <= 1).all():  # every prior is (1 - e^-lam) / (1 - e^-lam) * e^-0 = 1 exactly: P is a chain of the table's own bits
        out["pbound"] = 0.0
    nb = 12.0 * bps
    for k in range(K):
        if not P[k] > 0:
            continue
        i = int(lags[k])
        r = shift_of(c, i)
        f0 = float(sr) / (float(p_min + i) + r["shift"])
        x = nb * math.log2(f0 / fmin)
        tol = 3 * U if exact and r["shift"] == 0.0 else pm.f0_tolerance(c, r, L, p_min, p_max)
        xband = 2 * (nb * (tol + 4 * U) / math.log(2.0) + (abs(x) + 1.0) * 4 * U)
        if -1.0 < x < B + 1.0:
            marg.append(("rint", abs(x - math.floor(x) - 0.5), xband))
        b = int(min(max(np.rint(x), 0), B))
        out["x"][k] = x
        out["bins"][k] = b
        if b < B:
            obs[b] = P[k]  # ascending lag: the largest lag of a bin stays
    vp_sum = float(np.cumsum(obs)[-1])
    out["vp"] = min(max(vp_sum, 0.0), 1.0)
    out["vp_sum"] = vp_sum
    return out


def log_observation(obs, vp, B):
    """(2B,) log(observation + tiny) of one frame."""
    o = np.empty(2 * B)
    o[:B] = obs
    o[B:] = (1.0 - vp) / B
    return np.log(o + TINY)


def viterbi(log_obs, lt, dlo=None, dtab=0.0):
    """Step 7 densely over (2B)^2: log_obs (F, 2B), lt (2B, 2B) [source][target]. dict(states, score, value, ptr, margins), with
    margins on the optimal path only. dlo (F,): a bound on |log_obs(device) - log_obs(model)| per frame; dtab: on the table."""
    F, S2 = log_obs.shape
    value = np.zeros((F, S2))
    ptr = np.zeros((F, S2), np.int64)
    E = np.zeros(F)
    if dlo is None:
        dlo = np.zeros(F)
    if F == 0:
        return dict(states=np.zeros(0, np.int64), score=0.0, value=value, ptr=ptr, margins=[], E=E)
    linit = math.log(1.0 / S2 + TINY)
    value[0] = log_obs[0] + linit
    E[0] = dlo[0] + 2 * U * abs(linit) + 2 * U * float(np.abs(value[0]).max())
    for t in range(1, F):
        tr = value[t - 1][:, None] + lt  # [source][target]
        ptr[t] = np.argmax(tr, axis=0)
        best = tr[ptr[t], np.arange(S2)]
        value[t] = log_obs[t] + best
        E[t] = E[t - 1] + dlo[t] + dtab + 4 * U * float(np.abs(value[t]).max() + np.abs(value[t - 1]).max() + abs(LT))
    states = np.zeros(F, np.int64)
    states[-1] = int(np.argmax(value[-1]))
    for t in range(F - 2, -1, -1):
        states[t] = ptr[t + 1, states[t + 1]]
    marg = []
    last = value[-1]
    s = states[-1]
    near = np.flatnonzero(last >= last[s] - 2 * E[-1])
    near = near[near != s]
    if near.size == 0:
        marg.append(("final", float(last[s] - np.delete(last, s).max()) if S2 > 1 else np.inf, 2 * E[-1]))
    elif (last[near] == last[s]).all():  # equal values: the lower state wins on both sides
        marg.append(("final", np.inf, 0.0))
    else:
        marg.append(("final", 0.0, 2 * E[-1]))
    for t in range(1, F):
        j = states[t]
        col = value[t - 1] + lt[:, j]
        s = states[t - 1]
        bandt = 2 * E[t - 1] + 2 * dtab
        near = np.flatnonzero(col >= col[s] - bandt)
        near = near[near != s]
        # a tie of the same expression of the same bits (equal values, equal table entries) has band 0: the lower state wins
        same = (value[t - 1][near] == value[t - 1][s]) & (lt[near, j] == lt[s, j])
        if near.size == 0:
            marg.append(("ptr", float(col[s] - np.delete(col, s).max()) if S2 > 1 else np.inf, bandt))
        elif same.all():
            marg.append(("ptr", np.inf, 0.0))
        else:
            marg.append(("ptr", 0.0, bandt))
    return dict(states=states, score=float(value[-1, states[-1]]), value=value, ptr=ptr, margins=marg, E=E)


def path_score(states, log_obs, lt):
    """The score of a path under the model's tables."""
    if len(states) == 0:
        return 0.0
    v = log_obs[0, states[0]] + math.log(1.0 / log_obs.shape[1] + TINY)
    for t in range(1, len(states)):
        v = log_obs[t, states[t]] + (v + lt[states[t - 1], states[t]])
    return float(v)


def sum_error(vp_sum, pbound):
    """The absolute distance of two evaluations of the sum of a frame's observations (at most 2049 additions of non-negative terms);
    0 where the observations are the same bits on both sides (pbound 0): the chain is then the same too."""
    return 0.0 if pbound == 0.0 else (pbound + 4096 * U) * max(vp_sum, 0.0)


def decode(obs, w, switch_prob, dlo=None, unvoiced=None, lt=None):
    """Steps 5 (vp and the unvoiced observations), 6 and 7 on dense rows obs (F, B): the contract of vsyn_pyin_decode_device, whose
    vp is the same chain over the same bits. unvoiced (F,), where not NaN, replaces a frame's unvoiced observation (pyin below).
    dict(states, score, vp, log_obs, lt, margins, decided, E)."""
    obs = np.asarray(obs, np.float64)
    F, B = obs.shape
    vp = np.clip(np.cumsum(obs, axis=1)[:, -1], 0.0, 1.0) if F else np.zeros(0)
    lt = log_transition(B, w, switch_prob) if lt is None else lt
    log_obs = np.zeros((F, 2 * B))
    for f in range(F):
        log_obs[f] = log_observation(obs[f], vp[f], B)
        if unvoiced is not None and not np.isnan(unvoiced[f]):
            log_obs[f, B:] = math.log(unvoiced[f] + TINY)
    base = np.full(F, 4 * U * abs(LT))
    vit = viterbi(log_obs, lt, base if dlo is None else base + dlo, 2.0 ** -50 * abs(LT))
    return dict(states=vit["states"], score=vit["score"], vp=vp, log_obs=log_obs, lt=lt, margins=vit["margins"], E=vit["E"],
                decided=all(m > b for _, m, b in vit["margins"]))


def pyin(y, sr, fmin, fmax, beta, L=2048, H=512, lam=2.0, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01,
         center=True):
    """Steps 1 to 8 on the mono signal y (T,) float32 with the caller's table beta (N,): dict(f0 (F,) float64: the bin's frequency
    before the rounding to float32, voiced (F,) bool, vp (F,), states (F,), bins (F,): state mod B, score, obs (F, B), frames: the
    per-frame dicts of frame_observation, margins: every (frame or -1, name, margin, band), decided, B, w, bps, pbound, refused, dec:
    decode(obs) itself).

    The sum of a frame's observations is 1 in exact arithmetic whenever its lowest trough is below every threshold, so in float64 it
    lands on either side of 1, and (1 - vp) / B is then 0 on one side and about 1e-16 / B on the other: log(tiny) against about -43.
    Where the sum is a chain of the same bits on both sides (every n_m <= 1: all priors are exactly 1) nothing differs. Elsewhere
    such a frame is uncertain: the path is decided only if it is the optimum with the frame's unvoiced observation at the upper end
    of what the error admits AND is voiced in that frame. A path's score does not fall when an unvoiced observation rises, and this
    path's does not depend on it, so it is then the optimum for every value in between, and its margins at the upper end are the
    smallest."""
    y = np.asarray(y, np.float32)
    beta = np.asarray(beta, np.float64)
    N = beta.shape[0]
    p_min, p_max = pm.periods(sr, fmin, fmax, L)
    bps, B = num_bins(fmin, fmax, resolution)
    w = width(sr, H, max_transition_rate, bps)
    F = pm.num_frames(y.shape[0], L, H, center)
    out = dict(f0=np.zeros(F), voiced=np.zeros(F, bool), vp=np.zeros(F), states=np.zeros(F, np.int64), bins=np.zeros(F, np.int64), score=0.0,
               obs=np.zeros((F, B)), frames=[], margins=[], decided=True, B=B, w=w, bps=bps, p_min=p_min, p_max=p_max, refused=False,
               pbound=p_bound(N, 1, lam), dec=None)
    if not np.isfinite(y).all():
        out["refused"] = True
        out["f0"][:] = np.nan
        out["vp"][:] = np.nan
        return out
    if F == 0:
        return out
    thr = thresholds(N)
    band = pm.band(L, p_max)
    dlo = np.zeros(F)
    unvoiced = np.full(F, np.nan)
    for f, z in enumerate(pm.frames_of(y, L, H, center)):
        c, _ = pm.cmnd(z, p_min, p_max)
        fo = frame_observation(c, sr, p_min, float(fmin), bps, B, thr, beta, float(lam), float(no_trough_prob), band, pm.exact_frame(z), L, p_max)
        out["frames"].append(fo)
        out["obs"][f] = fo["obs"]
        out["pbound"] = max(out["pbound"], fo["pbound"])
        out["margins"] += [(f, nm, m, b) for nm, m, b in fo["margins"]]
        vs = fo.get("vp_sum", 0.0)
        e = sum_error(vs, fo["pbound"])
        dlo[f] = fo["pbound"]
        if e == 0.0 or vs > 1.0 + e:  # the same bits, or clipped on both sides
            pass
        elif vs < 1.0 - e:
            dlo[f] += e / (1.0 - vs - e) + 8 * U
        else:
            unvoiced[f] = 2.0 * e / B
    lt = log_transition(B, w, switch_prob)
    dec = decode(out["obs"], w, switch_prob, lt=lt)
    hi = decode(out["obs"], w, switch_prob, dlo, unvoiced, lt)
    out["dec"] = dec
    out["vp"] = dec["vp"]
    out["margins"] += [(-1, nm, m, b) for nm, m, b in hi["margins"]]
    unsure = ~np.isnan(unvoiced)
    if not np.array_equal(hi["states"], dec["states"]) or (hi["states"][unsure] >= B).any():
        out["margins"].append((-1, "vp", 0.0, np.inf))
    out["states"] = dec["states"]
    out["score"] = dec["score"]
    out["bins"] = dec["states"] % B
    out["voiced"] = dec["states"] < B
    out["f0"] = float(fmin) * 2.0 ** (out["bins"] / (12.0 * bps))
    out["unsure"] = unsure
    out["decided"] = all(m > b for _, _, m, b in out["margins"])
    return out
