"""The shapes at which the resampler's index arithmetic (csrc/vsyn_resample.h) is held to tests/resample_model.py: one seeded case
table that tests/test_resample_cases_cpu.py (the table's own promises, on the model) and tests/test_gpu_resample_shapes.py (the
device) share.

A case is one vsyn_resample_device call: its out_rate, per segment the in-rate (0 = skipped) and the frames, the channels, the
plane stride and the pointer offsets in floats. Under "reach" it states what it gets to: per pair the kernel variant, K4, the table
and span bytes; per variant the most chunks and tiles of a segment; the first tile whose 64-bit position c0 = j0 down + H is 2^32
or more; the first full tile whose input span is the bound rs_span4. Those statements are literals; reach(case) recomputes them by
the restatement of the host plan below (plan, tile_span4), and the CPU module compares the two, with RS_THREADS, RS_PER_THREAD,
RS_TILES and RS_LDS_BUDGET read from the header text, so that neither the table nor the restatement can drift from the kernel.

No test can read back which kernel variant ran: "lds", "global" and "copy" are the restatement's statement of what the host plan
chooses, nothing the device reports.

Two inputs per case.
    impulses  x is 0 but for 1.0 at a few positions of each plane (impulse_positions: 0, T - 1, the first and last input of a
              tile's span, either side of a chunk's first output), no two within K4 of each other in one plane, so that an output
              is exactly 0 or the one float32 tap: |y[j] - h[n]| <= 2^-23 |h[n]| with n = tap_index(j, p) (one float32 ulp: the
              device rounds its table from a C++ double, the model from numpy's), and exactly 0 where tap_index says none. This
              is the index check; it holds every (j, p) to its tap whatever K4 is.
    noise     uniform in [-1, 1] against resample / resample_at: 2e-6 max(1, max|x|) where K4 <= 64 (the gate of
              test_gpu_resample.py), else the chain's own bound B_j = (K4 + 2) 2^-24 sum_t |P[phi][t]| |x[i0 - t]| (bound): a
              chain of K4 fused multiply-adds over float32 taps. B_j is derived, not measured; a float32 multiply-add chain with
              two roundings per term stays inside it (CPU module). It cannot see a misplaced tap when K4 is large; the impulses do.
long_lds has one input: impulses, and a stretch of noise (case["stretch"]) between them."""
import functools
import zlib

import numpy as np

from tests import resample_model as rm

RS_THREADS, RS_PER_THREAD, RS_TILES = 256, 4, 8
RS_TILE = RS_THREADS * RS_PER_THREAD
RS_CHUNK = RS_TILE * RS_TILES
RS_LDS_BUDGET = 80 * 1024
GATE = 2e-6  # K4 <= 64
ULP = 2.0 ** -23
EDGES = (1023, 1024, 1025, 8191, 8192, 8193, 16384, 16385)  # T_out on a tile's and a chunk's edge


# ---- the host plan and the kernel's per-tile arithmetic, restated ----

def plan(r_in, r_out):
    """rs_build_table for one pair."""
    up, down = rm.ratio(r_in, r_out)
    p = dict(up=up, down=down, K4=0, H=0, N=0, span4=0, table_bytes=0, span_bytes=0, lds_bytes=0, variant="copy")
    if up == down:
        return p
    M = max(up, down)
    N = 20 * M + 1
    K4 = (-(-N // up) + 3) & ~3
    d = -(-(RS_TILE - 1) * down // up)
    span4 = (d + K4 + 3) // 4 + 1  # rs_span4
    lds = 4 * (up * K4 + 4 * span4)
    p.update(K4=K4, H=10 * M, N=N, span4=span4, table_bytes=4 * up * K4, span_bytes=16 * span4, lds_bytes=lds,
             variant="lds" if lds <= RS_LDS_BUDGET else "global")
    return p


def i0_of(p, j):
    return (np.asarray(j, np.int64) * p["down"] + p["H"]) // p["up"]


def tile_span4(p, tile, kn=RS_TILE):
    """The float4s that vsyn_rs_kernel<true> stages for the tile(s) starting at output tile * RS_TILE with kn outputs, before the
    min with span4: (e - a0) / 4 + 1."""
    c0 = np.asarray(tile, np.int64) * RS_TILE * p["down"] + p["H"]
    qb, rb = c0 // p["up"], c0 % p["up"]
    a0 = (qb - (p["K4"] - 1)) & ~np.int64(3)
    e = qb + (rb + (kn - 1) * p["down"]) // p["up"]
    return (e - a0) // 4 + 1


def span_period(p):
    """Tile starts after which (rb, qb mod 4), and so tile_span4, repeat."""
    return 4 * p["up"]


def first_tile_past_2_32(p, To):
    """The first tile of a segment of To outputs with c0 >= 2^32, or None."""
    j = -(-(2 ** 32 - p["H"]) // p["down"])
    k = -(-j // RS_TILE)
    return k if p["variant"] != "copy" and k * RS_TILE < To else None


def first_widest_tile(p, To):
    """The first full tile of a segment of To outputs whose span is span4, or None (the LDS variant alone stages a span)."""
    full = To // RS_TILE
    if p["variant"] != "lds" or not full:
        return None
    hit = np.flatnonzero(tile_span4(p, np.arange(min(full, span_period(p)))) == p["span4"])
    return int(hit[0]) if hit.size else None


def frames_for(r_in, r_out, To):
    """The fewest input frames that give To outputs."""
    up, down = rm.ratio(r_in, r_out)
    return (To - 1) * down // up + 1 if To else 0


# ---- the table ----

def _case(name, out_rate, in_rates, frames, channels=1, plane=None, in_off=0, out_off=0, out_pad=0, stretch=None, seed=None, reach=None):
    frames = [int(f) for f in frames]
    assert len(in_rates) == len(frames)
    return dict(name=name, out_rate=out_rate, in_rates=list(in_rates), frames=frames, channels=channels,
                plane=max(frames) if plane is None else plane, in_off=in_off, out_off=out_off, out_pad=out_pad, stretch=stretch, seed=seed or name, reach=reach)


_EDGE_RATES = (44100, 44056, 16000)
_MANY_S = 700
ALIGN_PLANES = (3008, 3009, 3010)  # 4k, 4k + 1, 4k + 2
ALIGNED = "align_p3008_i0_o0"


def _many_frames():
    rng = np.random.default_rng(700)
    return [int(v) for v in rng.choice([0, 1, 5, 300, 9000], _MANY_S)]


def _align_cases():
    out = []
    for si, pl in enumerate(ALIGN_PLANES):
        for io in range(4):
            oo = (io + si + (si > 0)) % 4  # every output offset against several input offsets; (4k, 0, 0) is the aligned run
            out.append(_case("align_p%d_i%d_o%d" % (pl, io, oo), 16000, [44100, 44056], [3005, 3008], channels=2, plane=pl, in_off=io,
                             out_off=oo, out_pad=pl % 4, seed="align",  # one input for all of them
                             reach=dict(pairs={44100: ("lds", 56, 35840, 11520), 44056: ("global", 56, 448000, 11520)},
                                        chunks=dict(lds=1, **{"global": 1}), tiles=dict(lds=2, **{"global": 2}), past32={}, widest={})))
    return out


CASES = [
    # 27 M frames of 44.1 kHz, 10 minutes: tiles from 9511 (output 9 739 264) on have c0 >= 2^32. Zeros, impulses and 50 000 noise
    # samples behind input 26.9 M, whose footprint lies past the crossing.
    _case("long_lds", 16000, [44100], [27_000_000], stretch=(26_900_000, 50_000),
          reach=dict(pairs={44100: ("lds", 56, 35840, 11520)}, chunks=dict(lds=1196), tiles=dict(lds=9567), past32={44100: 9511},
                     widest={44100: 1})),
    # up 65535, down 65536: a 6.3 MB table, c0 >= 2^32 from tile 64 on
    _case("long_global", 65535, [65536], [70_000],
          reach=dict(pairs={65536: ("global", 24, 6291360, 4208)}, chunks={"global": 9}, tiles={"global": 69}, past32={65536: 64},
                     widest={})),
    # the contract's limit max(up, down) = 65536, downwards: K4 = 1 310 724 taps per output
    _case("down_65536", 1, [65536, 65536, 65536, 65536], [3 * 65536 + 5, 2 * 65536, 3, 1], channels=4, plane=3 * 65536 + 8,
          reach=dict(pairs={65536: ("global", 1310724, 5242896, 273416224)}, chunks={"global": 1}, tiles={"global": 1}, past32={}, widest={})),
    # and upwards: every input sample becomes 65536 outputs
    _case("up_65536_from_1", 65536, [1, 1, 1], [3, 7, 1], channels=2, plane=8,
          reach=dict(pairs={1: ("global", 24, 6291456, 128)}, chunks={"global": 56}, tiles={"global": 448}, past32={}, widest={})),
    # 65535 / 65536 and a prime: 65521 / 65536
    _case("up_65536_near", 65536, [65535, 65521, 65535, 65521], [20000, 20000, 3, 3], channels=2,
          reach=dict(pairs={65535: ("global", 24, 6291456, 4208), 65521: ("global", 24, 6291456, 4208)}, chunks={"global": 3},
                     tiles={"global": 20}, past32={}, widest={})),
    # the LDS budget: 380 -> 31 needs exactly RS_LDS_BUDGET = 81920 bytes (the LDS variant at equality), 204 -> 13 needs 81936
    _case("budget_lds", 31, [380, 380], [frames_for(380, 31, 3000), frames_for(380, 31, 20000)],
          reach=dict(pairs={380: ("lds", 248, 30752, 51168)}, chunks=dict(lds=3), tiles=dict(lds=20), past32={}, widest={380: 0})),
    _case("budget_global", 13, [204, 204], [frames_for(204, 13, 3000), frames_for(204, 13, 20000)],
          reach=dict(pairs={204: ("global", 316, 16432, 65504)}, chunks={"global": 3}, tiles={"global": 20}, past32={}, widest={})),
    # T_out on every tile and chunk edge, per variant; 16385 outputs are three chunks
    _case("edges", 16000, [r for r in _EDGE_RATES for _ in EDGES], [frames_for(r, 16000, To) for r in _EDGE_RATES for To in EDGES],
          reach=dict(pairs={44100: ("lds", 56, 35840, 11520), 44056: ("global", 56, 448000, 11520), 16000: ("copy", 0, 0, 0)},
                     chunks=dict(lds=3, copy=3, **{"global": 3}), tiles=dict(lds=17, copy=17, **{"global": 17}), past32={},
                     widest={44100: 1})),
    # 22050 -> 16000 reaches its widest span first in tile 4, which 7056 input frames fill
    _case("widest_span", 16000, [22050, 22050], [7056, 9000],
          reach=dict(pairs={22050: ("lds", 28, 35840, 5776)}, chunks=dict(lds=1), tiles=dict(lds=7), past32={}, widest={22050: 4})),
    # what the pitch shift asks for: rint(sr / rate) -> sr, 11025 / 9271, over three chunks
    _case("pitch_pair", 44100, [37084], [14000],
          reach=dict(pairs={37084: ("global", 24, 1058400, 3568)}, chunks={"global": 3}, tiles={"global": 17}, past32={}, widest={})),
] + _align_cases() + [
    # both scans' second pass (S > 256), the binary search over runs of equal offsets (empty and skipped segments), both variants and
    # the copy interleaved
    _case("many_segments", 16000, [(44100, 44056, 16000, 0)[g % 4] for g in range(_MANY_S)], _many_frames(), channels=2, plane=9000,
          reach=dict(pairs={44100: ("lds", 56, 35840, 11520), 44056: ("global", 56, 448000, 11520), 16000: ("copy", 0, 0, 0)},
                     chunks=dict(lds=1, copy=2, **{"global": 1}), tiles=dict(lds=4, copy=9, **{"global": 4}), past32={},
                     widest={44100: 1})),
    # frames[g] above the plane stride: clamped to the plane
    _case("frames_past_plane", 16000, [44100, 44056, 16000], [4000, 4000, 4000], channels=2, plane=3000,
          reach=dict(pairs={44100: ("lds", 56, 35840, 11520), 44056: ("global", 56, 448000, 11520), 16000: ("copy", 0, 0, 0)},
                     chunks=dict(lds=1, copy=1, **{"global": 1}), tiles=dict(lds=2, copy=3, **{"global": 2}), past32={},
                     widest={})),
    _case("channels_255", 16000, [44100], [300], channels=255,
          reach=dict(pairs={44100: ("lds", 56, 35840, 11520)}, chunks=dict(lds=1), tiles=dict(lds=1), past32={}, widest={})),
]
BY_NAME = {c["name"]: c for c in CASES}
IDS = [c["name"] for c in CASES]


def seg_frames(case, g):
    """T: the frames the device reads of segment g (clamped to the plane)."""
    return min(case["frames"][g], case["plane"])


def seg_out_frames(case, g):
    r = case["in_rates"][g]
    return rm.num_frames(r, case["out_rate"], seg_frames(case, g)) if r else 0


def out_plane(case):
    """The smallest out_plane_stride the call accepts (every pair at T = plane), plus the case's padding."""
    return max(rm.num_frames(r, case["out_rate"], case["plane"]) for r in case["in_rates"] if r) + case["out_pad"]


def reach(case):
    """What the case's literals state, recomputed from the restatement."""
    pairs, chunks, tiles, past32, widest = {}, {}, {}, {}, {}
    for g, r in enumerate(case["in_rates"]):
        if not r:
            continue
        p = plan(r, case["out_rate"])
        v, To = p["variant"], seg_out_frames(case, g)
        pairs[r] = (v, p["K4"], p["table_bytes"], p["span_bytes"])
        chunks[v] = max(chunks.get(v, 0), -(-To // RS_CHUNK))
        tiles[v] = max(tiles.get(v, 0), -(-To // RS_TILE))
        k = first_tile_past_2_32(p, To)
        if k is not None:
            past32[r] = min(k, past32.get(r, k))
        k = first_widest_tile(p, To)
        if k is not None:
            widest[r] = min(k, widest.get(r, k))
    return dict(pairs=pairs, chunks=chunks, tiles=tiles, past32=past32, widest=widest)


# ---- inputs ----

@functools.lru_cache(maxsize=None)
def tables(r_in, r_out):
    """(h float64 [N], P float64 [up][K4]) of the model."""
    up, down = rm.ratio(r_in, r_out)
    h = rm.taps(up, down)
    return h, rm.polyphase(up, down, h)


def _seed(case, what):
    return zlib.crc32(("%s/%s" % (case["seed"], what)).encode())


def impulse_positions(r_in, r_out, T):
    """Input positions worth an impulse, most wanted first: 0 and T - 1; the first input (the last tap of its first output) and the
    last input of the span of tile 1, of the last tile, of the first tile past 2^32 and of the first widest tile; the input under
    the first output of chunk 1 and of the last chunk, and the one behind it."""
    p = plan(r_in, r_out)
    To = rm.num_frames(r_in, r_out, T)
    if T == 0:
        return []
    out = [0, T - 1]
    if p["variant"] == "copy":
        out += [q for jc in (RS_CHUNK, (To - 1) // RS_CHUNK * RS_CHUNK) for q in (jc - 1, jc)]
    else:
        last = (To - 1) // RS_TILE
        for k in (first_tile_past_2_32(p, To), first_widest_tile(p, To), min(1, last), last):
            if k is not None:
                j0 = k * RS_TILE
                out += [int(i0_of(p, j0)) - (p["K4"] - 1), int(i0_of(p, min(j0 + RS_TILE, To) - 1))]
        for jc in (RS_CHUNK, (To - 1) // RS_CHUNK * RS_CHUNK):
            if 0 < jc < To:
                out += [int(i0_of(p, jc)), int(i0_of(p, jc)) + 1]
    seen = []
    for q in out:
        q = min(max(q, 0), T - 1)
        if q not in seen:
            seen.append(q)
    return seen


def impulse_planes(case, g):
    """Per channel the impulse positions of segment g: impulse_positions dealt over the channels, most wanted first, each into the
    first plane (from the one whose turn it is) where it is K4 or more from every impulse already there; one that fits nowhere is
    left out. So no output of a plane sees two impulses."""
    r, C = case["in_rates"][g], case["channels"]
    planes = [[] for _ in range(C)]
    if not r:
        return planes
    sep = max(plan(r, case["out_rate"])["K4"], 1)
    for n, q in enumerate(impulse_positions(r, case["out_rate"], seg_frames(case, g))):
        for c in range(min(C, 8)):
            pl = planes[(n + c) % min(C, 8)]
            if all(abs(q - o) >= sep for o in pl):
                pl.append(q)
                break
    if C > 8:  # channels_255: every plane gets impulses, the planes past 8 those of plane c % 8
        for c in range(8, C):
            planes[c] = list(planes[c % 8])
    return planes


def stretch_noise(case):
    a, n = case["stretch"]
    return np.random.default_rng(_seed(case, "stretch")).uniform(-1.0, 1.0, n).astype(np.float32)


def impulse_input(case):
    """float32 [S][C][plane]: zeros, 1.0 at impulse_planes, the stretch of noise where the case has one; NaN behind each segment's
    frames when the plane is longer (the device must not read it)."""
    S, C = len(case["frames"]), case["channels"]
    x = np.zeros((S, C, case["plane"]), np.float32)
    for g in range(S):
        for c, pl in enumerate(impulse_planes(case, g)):
            x[g, c, pl] = 1.0
        x[g, :, seg_frames(case, g):] = np.nan
    if case["stretch"]:
        a, n = case["stretch"]
        x[0, 0, a:a + n] = stretch_noise(case)
    return x


def noise_input(case):
    """float32 [S][C][plane], uniform in [-1, 1]; NaN behind each segment's frames."""
    S, C = len(case["frames"]), case["channels"]
    n = max(seg_frames(case, g) for g in range(S))  # drawn at the longest segment's length, so that the plane stride changes no value
    x = np.full((S, C, case["plane"]), np.nan, np.float32)
    x[:, :, :n] = np.random.default_rng(_seed(case, "noise")).uniform(-1.0, 1.0, (S, C, n))
    for g in range(S):
        x[g, :, seg_frames(case, g):] = np.nan
    return x


# ---- what the outputs must be ----

def footprint(r_in, r_out, T, a, b):
    """[lo, hi): the outputs that read an input of [a, b)."""
    p = plan(r_in, r_out)
    To = rm.num_frames(r_in, r_out, T)
    lo = -(-(a * p["up"] - p["H"]) // p["down"])  # the first j with i0 >= a
    hi = ((b - 1 + p["K4"]) * p["up"] - 1 - p["H"]) // p["down"] + 1  # behind the last j with i0 - K4 + 1 <= b - 1
    return min(max(lo, 0), To), min(max(hi, 0), To)


def impulse_outputs(r_in, r_out, T, positions):
    """(j, want): the outputs that the impulses of one plane reach, ascending, and the float64 tap h[tap_index(j, p)] each must be;
    every other output of the plane is exactly 0."""
    h, _ = tables(r_in, r_out)
    js, ws = [], []
    for q in sorted(positions):
        lo, hi = footprint(r_in, r_out, T, q, q + 1)
        j = np.arange(lo, hi, dtype=np.int64)
        n = rm.tap_index(r_in, r_out, j, q)
        js.append(j[n >= 0])
        ws.append(h[n[n >= 0]])
    j = np.concatenate(js) if js else np.zeros(0, np.int64)
    assert (np.diff(j) > 0).all(), "two impulses under one output"
    return j, (np.concatenate(ws) if ws else np.zeros(0))


def check_impulses(y, r_in, r_out, T, positions, what, skip=None):
    """y float32 [T_out] of one plane against impulse_outputs; skip = (lo, hi) leaves those outputs to the caller (long_lds).
    Returns the largest |y - h[n]| / (2^-23 |h[n]|)."""
    want = np.zeros(y.shape[0])
    j, w = impulse_outputs(r_in, r_out, T, positions)
    want[j] = w
    yy = y.astype(np.float64)
    if skip:
        assert not want[skip[0]:skip[1]].any(), what
        yy[skip[0]:skip[1]] = 0.0
    zero = want == 0
    bad = np.flatnonzero(zero & (yy != 0))
    assert not bad.size, (what, "outputs that no impulse reaches are not 0", bad[:8], yy[bad[:8]])
    d = np.abs(yy[~zero] - want[~zero]) / (ULP * np.abs(want[~zero]))
    worst = float(d.max(initial=0.0))
    assert worst <= 1.0, (what, worst, np.flatnonzero(~zero)[np.argmax(d)])
    return worst


def bound(x, r_in, r_out, j):
    """B_j = (K4 + 2) 2^-24 sum_t |P[phi][t]| |x[i0 - t]| at the outputs j of one plane x."""
    _, P = tables(r_in, r_out)
    return (P.shape[1] + 2) * 2.0 ** -24 * rm.resample_at(np.abs(x), r_in, r_out, j, P=np.abs(P))


def check_noise(y, x, r_in, r_out, what, j=None):
    """y float32 [len(j)] (j = None: every output) of one plane x [T] against the model. Returns (|d| / gate at its worst, "flat" or
    "chain": which gate the pair has)."""
    p = plan(r_in, r_out)
    if p["variant"] == "copy":
        assert j is None and np.array_equal(y.view(np.uint32), x.view(np.uint32)), what
        return 0.0, "copy"
    j = np.arange(rm.num_frames(r_in, r_out, x.shape[0]), dtype=np.int64) if j is None else j
    assert y.shape == j.shape, (what, y.shape, j.shape)
    if not j.size:
        return 0.0, "flat"
    d = np.abs(y.astype(np.float64) - rm.resample_at(x, r_in, r_out, j, P=tables(r_in, r_out)[1]))
    if p["K4"] <= 64:
        kind, r = "flat", d / (GATE * max(1.0, float(np.abs(x).max())))
    else:
        kind, r = "chain", d / bound(x, r_in, r_out, j)
    worst = float(r.max())
    assert worst <= 1.0, (what, kind, worst, int(j[np.argmax(r)]))
    return worst, kind
