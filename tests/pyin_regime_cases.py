"""The inputs of tests/test_gpu_pyin_regimes.py: the pyin kernels (csrc/vsyn_pyin.h) at the sizes where B, N and the trough count K
leave one stride of a thread loop, shared with tests/test_pyin_regimes_cpu.py, which asserts on the CPU, from the model alone
(tests/pyin_model.py), that every case is decided and reaches the branch it is there for. Everything comes from fixed seeds; the
model's results are memoised per regime.

A. DECODE: regimes of vsyn_pyin_decode_device (1024 threads, 4 states and 2 scan elements a thread), one spec and one launch each.
   BW lists (B, w) per rate, as computed with pyin_model.num_bins and width; the CPU module asserts them.
     stride2   B 1201 (2B = 2402: the strides q = 0 .. 2, 10 of the 16 waves hold a scan element); a second rate gives w = 101.
     stride3   B 2048 (2B = 4096: q = 0 .. 3, all 16 waves, states up to 4095 in the 2-byte back pointers and scan states).
     h0_few    w = 1 (h = 0: no edge row, a band of one entry) at B 12; the second rate gives w = 3.
     h0_many   w = 1 at B 601 (max_transition_rate 1).
     no_oob    B 59 <= h + 1 = 71: no target has a source outside its band, the scans do not run.
     b_h1 b_h2 B = h + 1 = 36 (still no such source) and B = h + 2 = 37 (targets 0 and B - 1 have exactly one).
     b_wm1 b_w b_wp1   B = w - 1, w, w + 1 = 70, 71, 72: every row an edge row; one interior source; two.
     long      B 12, w 3 with F = 1100 (the vp pass of the decode entry takes two strides of 1024 frames) and F = 1.
     sw03 sw049  switch_prob 0.3 (on b_wp1's sizes) and 0.49 (on B 12, w 3).
   Row kinds (rows_of), every row's sum at most 1:
     sparse    three random bins a frame, sum below 1 (the path mostly waits in unvoiced states).
     alternate all mass (1.0: vp == 1, a clean voiced jump) in bin 0, twice in B - 1, then in 0: the prefix and the suffix maximum
               travel the whole range. (A jump costs log tiny, as much as sitting out one frame on a zero observation, so in the
               middle of a segment the mass stays for two frames where the path is to follow it; in the last frame one is enough,
               since staying behind costs the zero observation and a transition.)
     up down   1.0 in a source bin s, then in s + h + 1 (s - h - 1): s is the LAST element of the target's prefix (the FIRST of
               its suffix). s = m and m - 1 for multiples m of 128: the first element of a wave and the last of the one below,
               below and above bin 1024.
     up_far    the same with a jump of h + 1 + 64: the source lies in the wave next to the one whose element is looked up (its last
     down_far  element below for up_far, its first element above for down_far), and so arrives through that wave's total alone.
     tie_hi    0.5 in a and b = a + 1 (in two waves where B allows), then 1.0 in b + h + 1 (tie_lo: in a - h - 1): the two
     tie_lo    sources tie in every bit (equal values, both transitions log tiny) and the lower state has to win through the
               waves' totals, in the prefix and in the suffix scan. tie_hi_far, tie_lo_far: a jump of h + 1 + 192, so that both
               sources arrive through the totals of two different waves.
     pair      pyin_cases' "pair": 0.25 in a and its mirror image B - 1 - a on every frame; two paths tie, the lower wins.
     vtie      one frame whose only voiced value x equals its unvoiced value (1 - x) / B in every bit: voiced state i ties with
               ALL unvoiced states B .. 2B - 1 (every stride and wave of the final arg-max) and wins as the lowest.
     unv_hi    1.0 in B - 1, a zero row, 1.0 in an interior bin c far below: the path is B - 1, 2B - 1, c, so the out-of-band
     unv_lo    source of c is the highest state there is, through the suffix scan and a back pointer. Mirrored: 0, B, c. (The
               edge bin's own loc entry is about twice an interior one's, which decides against "jump, then switch".)
     unv_end   1.0 in B - 1 and a zero row: the path ends in state 2B - 1, the last thread's last stride of the final arg-max.
     dense     every bin random, sum below 1; "low" and "high" put nine tenths of the mass within h + 2 bins of an edge, so that
               the edge rows and both clamps of the in-band walk carry the decision.

B. STAGE: cases of vsyn_pyin_device that move the observation kernel (256 threads) off its one stride.
     n1 n256 n257 n1024   n_thresholds N with beta_probs(N): the tile holds TR = 64, 11, 11, 2 troughs. 100 .. 400 Hz at (512, 128):
               61 lags at 8000 Hz, 121 at 16000 Hz. A tone (few troughs), noise (many) and a tone at the other rate.
     k410      44100 Hz, (2048, 512), 44 .. 1500 Hz (lags 29 .. 1003, B 611): an 11 kHz sine in noise, a trough every fourth lag.
     k690      (4096, 1024), 22 .. 1500 Hz (lags 29 .. 2005, B 731): noise.
     k_coarse  k410's signal at resolution 0.5 (B 123): neighbouring candidates share a bin across k = 256.
     lam05 lam8  (boltzmann_parameter, no_trough_prob) = (0.5, 0.0) and (8.0, 1.0) on a two-step tone, 200 .. 280 Hz at (512, 128).
"""
import functools

import numpy as np

from tests import pyin_cases as yc
from tests import pyin_model as ym
from tests import trim_model as tm

C2, C7 = yc.C2, yc.C7
FMAX_2048 = C2 * 2.0 ** (2047.5 / 408.0)  # 12 * 34 bins an octave: B = floor(2047.5) + 1
FMAX_2049 = C2 * 2.0 ** (2048.5 / 408.0)
MTR, SW = 35.92, 0.01


def _dec(rates, L, H, fmin, fmax, resolution, BW, kinds, mtr=MTR, sw=SW, F=8):
    return dict(rates=rates, L=L, H=H, fmin=fmin, fmax=fmax, resolution=resolution, BW=BW, kinds=kinds, mtr=mtr, sw=sw, F=F)


def _k(*names):
    return tuple((k, 0, 0) for k in names)


_EDGE = _k("sparse", "alternate", "pair", "vtie", "dense", "low", "high")
# kinds: (kind, index of the rate, argument)
DECODE = {
    "stride2": _dec((22050, 44100), 2048, 512, C2, C7, 0.05, ((1201, 201), (1201, 101)),
                    _k("sparse", "alternate") + (("up", 0, 640), ("down", 0, 640), ("up", 0, 1024), ("down", 0, 1024), ("up", 0, 1023), ("down", 0, 1023),
                                                 ("up_far", 0, 639), ("down_far", 0, 640), ("tie_hi_far", 0, 640), ("tie_lo_far", 0, 640), ("tie_hi", 0, 640),
                                                 ("tie_lo", 0, 640)) + _k("pair", "vtie", "unv_hi", "unv_lo", "unv_end")
                    + (("sparse", 1, 1), ("tie_hi", 1, 1024), ("tie_lo", 1, 1024)), F=4),
    "stride3": _dec((22050,), 2048, 512, C2, FMAX_2048, 0.03, ((2048, 341),),
                    _k("sparse", "alternate") + (("up_far", 0, 1791), ("down_far", 0, 1792), ("tie_hi", 0, 1024), ("tie_lo", 0, 1024))
                    + _k("vtie", "unv_hi", "unv_end"), F=3),
    "h0_few": _dec((22050, 8000), 64, 16, 1000.0, 1400.0, 0.5, ((12, 1), (12, 3)),
                   _k("sparse", "alternate", "pair", "vtie", "dense") + (("up", 0, 5), ("down", 0, 5), ("sparse", 1, 1), ("alternate", 1, 0), ("unv_hi", 1, 0))),
    "h0_many": _dec((22050,), 2048, 512, C2, C7, 0.1, ((601, 1),),
                    _k("sparse", "alternate") + (("up", 0, 128), ("down", 0, 128), ("up", 0, 511), ("down", 0, 511), ("up_far", 0, 127), ("down_far", 0, 128))
                    + _k("pair", "vtie"), mtr=1.0, F=6),
    "no_oob": _dec((8000,), 512, 256, 200.0, 280.0, 0.1, ((59, 141),), _EDGE),
    "b_h1": _dec((8000,), 512, 128, 200.0, 245.0, 0.1, ((36, 71),), _EDGE),
    "b_h2": _dec((8000,), 512, 128, 200.0, 247.0, 0.1, ((37, 71),), _EDGE),
    "b_wm1": _dec((8000,), 512, 128, 200.0, 298.0, 0.1, ((70, 71),), _EDGE),
    "b_w": _dec((8000,), 512, 128, 200.0, 300.5, 0.1, ((71, 71),), _EDGE),
    "b_wp1": _dec((8000, 16000), 512, 128, 200.0, 302.0, 0.1, ((72, 71), (72, 31)), _EDGE + (("dense", 1, 1), ("tie_hi", 1, 0), ("tie_lo", 1, 0))),
    "long": _dec((8000,), 64, 16, 400.0, 550.0, 0.5, ((12, 3),), (("long", 0, 1100), ("long", 0, 1), ("sparse", 0, 0))),
    "sw03": _dec((8000, 16000), 512, 128, 200.0, 302.0, 0.1, ((72, 71), (72, 31)),
                 _EDGE + (("dense", 1, 1), ("tie_hi", 1, 0), ("tie_lo", 1, 0), ("unv_lo", 1, 0)), sw=0.3),
    "sw049": _dec((8000,), 64, 16, 400.0, 550.0, 0.5, ((12, 3),),
                  (("sparse", 0, 1),) + _k("alternate", "tie_hi", "tie_lo", "pair", "vtie", "unv_hi", "unv_lo", "dense"), sw=0.49),
}
LARGE = ("stride2", "stride3")
FAR, TIE_FAR = 64, 192  # bins beyond h + 1 that the "far" kinds jump
H0 = ("h0_few", "h0_many")


def spec(g):
    """The C spec of a decode regime or of a stage group."""
    from parseoggvorbis_amd import pitch
    return pitch.pyin_spec(fmin=g["fmin"], fmax=g["fmax"], frame_length=g["L"], hop_length=g["H"], resolution=g["resolution"], n_thresholds=g.get("N", 100),
                           boltzmann_parameter=g.get("lam", 2.0), no_trough_prob=g.get("ntp", 0.01), max_transition_rate=g.get("mtr", MTR),
                           switch_prob=g.get("sw", SW))


def _one(F, B, bins, value=1.0):
    o = np.zeros((F, B))
    for t, b in enumerate(bins):
        for x in np.atleast_1d(b):
            o[t, x] = value if np.ndim(b) == 0 else value / len(b)
    return o


def tie_value(B):
    """x with (1.0 - x) / B == x in float64, bit for bit (near 1 / (B + 1))."""
    x = 1.0 / (B + 1.0)
    for _ in range(64):
        for c in (x, np.nextafter(x, 0.0), np.nextafter(x, 1.0)):
            if (1.0 - c) / B == c:
                return float(c)
        x = (1.0 - x) / B
    raise AssertionError("no fixed point of (1 - x) / B at B = %d" % B)


def rows_of(kind, B, h, F, seed, arg):
    """(F', B) float64 observation rows of one segment."""
    rng = np.random.default_rng(20261021 + 7919 * seed + (1000003 * arg if kind == "sparse" else 0))
    if kind == "sparse":
        o = np.zeros((F, B))
        for t in range(F):
            o[t, rng.choice(B, 3, replace=False)] = rng.uniform(0.05, 0.3, 3)
        return o
    if kind == "alternate":
        return _one(4, B, [0, B - 1, B - 1, 0])
    if kind in ("up", "down", "up_far", "down_far"):
        d = h + 1 + (FAR if kind.endswith("far") else 0)
        to = arg + d if kind.startswith("up") else arg - d
        assert 0 <= to < B
        return _one(2, B, [arg, to])
    if kind in ("tie_hi", "tie_lo", "tie_hi_far", "tie_lo_far"):
        b = arg if arg else B // 2
        a = b - 1
        d = h + 1 + (TIE_FAR if kind.endswith("far") else 0)
        to = b + d if kind.startswith("tie_hi") else a - d
        assert 0 <= to < B
        return _one(2, B, [(a, b), to])
    if kind == "pair":
        a = max(0, B // 2 - 1 - h // 2)
        o = np.zeros((min(F, 7), B))
        o[:, a] = o[:, B - 1 - a] = 0.25
        return o
    if kind == "vtie":
        return _one(1, B, [(2 * B) // 3], tie_value(B))
    if kind in ("unv_hi", "unv_lo"):
        assert h >= 1 and h + 1 < B - 1 - 2 * h
        c = h + 1 if kind == "unv_hi" else B - 2 - h
        o = _one(4, B, [B - 1 if kind == "unv_hi" else 0, 0, c, c])
        o[1] = 0.0
        return o[:max(F, 3)]
    if kind == "unv_end":
        return np.vstack([_one(1, B, [B - 1]), np.zeros((1, B))])
    if kind in ("dense", "low", "high"):
        o = rng.uniform(0.01, 1.0, (F, B))
        if kind != "dense":
            near = np.arange(B) < h + 2 if kind == "low" else np.arange(B) >= B - h - 2
            o = np.where(near[None, :], o, o / (9.0 * max(1, B - near.sum()) / max(1, near.sum())))
        return o * (rng.uniform(0.5, 0.95, (F, 1)) / o.sum(axis=1, keepdims=True))
    if kind == "long":  # arg frames: every bin random; in every 37 frames all mass twice in bin 1, then twice in bin B - 2
        o = rng.uniform(0.01, 1.0, (arg, B))
        o *= rng.uniform(0.9, 0.99, (arg, 1)) / o.sum(axis=1, keepdims=True)
        for t in range(arg):
            if t % 37 >= 33:
                o[t] = 0.0
                o[t, 1 if t % 37 < 35 else B - 2] = 1.0
        return o
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def decode_segments(name):
    """The segments of one regime: a list of dict(kind, arg, sr, B, w, obs)."""
    r = DECODE[name]
    out = []
    for k, (kind, ri, arg) in enumerate(r["kinds"]):
        B, w = r["BW"][ri]
        out.append(dict(kind=kind, arg=arg, sr=r["rates"][ri], B=B, w=w, obs=rows_of(kind, B, w // 2, r["F"], 100 * list(DECODE).index(name) + k, arg)))
    return out


@functools.lru_cache(maxsize=None)
def _log_table(B, w, sw):
    return ym.log_transition(B, w, sw)


@functools.lru_cache(maxsize=None)
def decode_models(name):
    """pyin_model.decode of every segment of the regime (the dense log table is built once per (B, w))."""
    return [ym.decode(s["obs"], s["w"], DECODE[name]["sw"], lt=_log_table(s["B"], s["w"], DECODE[name]["sw"])) for s in decode_segments(name)]


# ---- B. the observation kernel ----

WIDE = dict(L=512, H=128, fmin=100.0, fmax=400.0, resolution=0.1)
STAGE = {
    "n1": dict(WIDE, N=1), "n256": dict(WIDE, N=256), "n257": dict(WIDE, N=257), "n1024": dict(WIDE, N=1024),
    "k410": dict(L=2048, H=512, fmin=44.0, fmax=1500.0, resolution=0.1),
    "k690": dict(L=4096, H=1024, fmin=22.0, fmax=1500.0, resolution=0.1),
    "k_coarse": dict(L=2048, H=512, fmin=44.0, fmax=1500.0, resolution=0.5),
    "lam05": dict(WIDE, lam=0.5, ntp=0.0), "lam8": dict(WIDE, lam=8.0, ntp=1.0),
}
for _g in STAGE.values():
    _g.setdefault("N", 100)
    _g.setdefault("lam", 2.0)
    _g.setdefault("ntp", 0.01)
T_N = 2500


def tile_rows(N):
    """TR of the observation kernel: min(64, 24576 / (8 (N | 1)))."""
    return max(1, min(64, 24576 // (8 * (N | 1))))


SINE_HZ = 14000.0


def _sine_in_noise(T, sr, seed):
    rng = np.random.default_rng(20261021 + seed)
    return (0.5 * np.sin(2 * np.pi * SINE_HZ * np.arange(T) / sr) + 0.05 * rng.standard_normal(T)).astype(np.float32)


def _noise(T, seed, amp=0.3):
    return (amp * np.random.default_rng(20261021 + seed).standard_normal(T)).astype(np.float32)


def _pure(T, sr, f, seed):
    """One sine with a trace of noise: one trough, or two."""
    rng = np.random.default_rng(20261021 + seed)
    return (0.5 * np.sin(2 * np.pi * f * np.arange(T) / sr) + 1e-4 * rng.standard_normal(T)).astype(np.float32)


# (group, kind, C, T, sr, seed)
_PLAN = [(g, k, c, T_N, sr, s) for g, s0 in (("n1", 4), ("n256", 10), ("n257", 20), ("n1024", 30))
         for k, c, sr, s in (("pure", 1, 8000, s0), ("noise", 1, 8000, s0 + 1), ("tone", 2, 16000, s0 + 2), ("noise", 3, 16000, s0 + 3))]
_PLAN += [("k410", "sine", 1, 4097, 44100, 40), ("k410", "sine", 2, 4097, 44100, 41), ("k690", "noise", 1, 3 * 4096, 44100, 50),
          ("k_coarse", "sine", 3, 4097, 44100, 60),
          ("lam05", "tone", 1, 4097, 8000, 70), ("lam05", "tone", 2, 4097, 16000, 71), ("lam8", "tone", 1, 4097, 8000, 72), ("lam8", "tone", 3, 4097, 16000, 73)]
_TONES = {"n1": (130.0, 260.0), "n256": (130.0, 260.0), "n257": (130.0, 260.0), "n1024": (130.0, 260.0), "lam05": (130.0, 260.0), "lam8": (120.0, 180.0)}
_PURE = {"n1": 113.0, "n256": 113.0, "n257": 113.0, "n1024": 113.0}


def _signal(grp, kind, T, sr, seed):
    if kind == "pure":
        return _pure(T, sr, _PURE[grp], seed)
    if kind == "tone":
        return yc.tone(T, sr, _TONES[grp], 5000 + seed)
    if kind == "sine":
        return _sine_in_noise(T, sr, seed)
    return _noise(T, seed)


@functools.lru_cache(maxsize=None)
def stage_cases():
    """A list of dict(group, kind, C, T, sr, x (C, T), and the group's spec fields)."""
    out = []
    for grp, kind, Cn, T, sr, seed in _PLAN:
        x = np.ascontiguousarray(np.stack([_signal(grp, kind, T, sr, seed * 4 + c) for c in range(Cn)]), np.float32)
        out.append(dict(STAGE[grp], group=grp, kind=kind, C=Cn, T=T, sr=sr, x=x))
    return out


@functools.lru_cache(maxsize=None)
def beta(N):
    from parseoggvorbis_amd.pitch import beta_probs
    return beta_probs(N, (2, 18))


@functools.lru_cache(maxsize=None)
def stage_models(group):
    """pyin_model.pyin of every case of the group, on the float32 downmix the device computes."""
    return [ym.pyin(tm.downmix(c["x"]), c["sr"], c["fmin"], c["fmax"], beta(c["N"]), c["L"], c["H"], lam=c["lam"], resolution=c["resolution"],
                    no_trough_prob=c["ntp"]) for c in stage_cases() if c["group"] == group]


def stage_group(group):
    return [c for c in stage_cases() if c["group"] == group]
