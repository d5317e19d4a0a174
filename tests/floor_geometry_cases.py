"""Floor-1 X lists whose x[1] differs from half the block size, as ONE seeded case table for test_oracle_vs_ref.py,
test_floor_geometry_cpu.py, test_gpu_floor_geometry.py and oracle/make_ref_vectors.py (goldens and tests cannot drift apart), and a
plain integer model of the floor-1 tail (hpp:521-589) in Python ints that shares no code with the oracle. numpy only, no GPU.

The format sets x[1] = 1 << rangebits (hpp:447-450) whatever the block size, so inner posts may lie anywhere below 2^rangebits, up to
32767. A floor vector holds n values of which the first n/2 are used (hpp:574, 1243-1255); a segment that ends beyond them is cut
(render_line, Utils.hpp:159-161), a curve whose last post lies below them is extended flat (hpp:583-584), and a floor that both
modes use always sees one of the two.

Geometries, per block-size pair (h0, h1 = half the short / long block; h = the half of the floor's own block):
  beyond2          x[1] = 2 h on both floors, 12..20 posts, posts at h - 1, h, h + 1, at least three more beyond h + 1
  beyond_max_a     x[1] = 32768, the two end posts only: one segment of adx 32768
  beyond_max_b     x[1] = 32768, 20 posts: nine inside the block, nine in 20000..32767 (a segment that crosses h has adx > 16384)
  short_of_half    x[1] = h / 2: flat over the upper half of the block
  short_of_quarter x[1] = h / 4
  short_of_one     xs = [0, 1]: flat from bin 1 on
  shared_long      ONE floor with x[1] = h1 for both modes: short blocks see posts far beyond h0 (h0 - 1, h0, h0 + 1 among them)
  shared_short     ONE floor with x[1] = h0 for both modes: long blocks are flat beyond h0
  steep            x[1] = h, the usual domain at its extremes: posts 0 1 2 3 and h-3 h-2 h-1 h (adx 1), and post 1 first in header
                   order, so that a row which codes only that post renders the pair (1, h)

Every setup carries each floor with all four multipliers (a mode per block size and multiplier), so that one batch holds rows of every
multiplier. Rows: random valid ones (random in-range targets, three in ten posts left at their prediction, like valid_ys of
test_oracle_vs_ref.py) and, per multiplier, eight directed ones (top = range - 1; top * multiplier = 255, 254, 255, 252):
  ends_top_0 / ends_0_top / ends_top_top   every inner code 0: the end posts alone are flagged
  alternate_0 / alternate_1                every post coded, sorted neighbours alternating 0 and top (phase 0 / 1)
  single_first / single_mid / single_last  one coded inner post (at that sorted position) among codes of 0, pushed to the far edge
Every row is one the reference decodes: the encoder below only emits codes whose unwrap stays in range."""
import numpy as np

from parseoggvorbis_amd.binding import PACKET_DTYPE, SEGMENT_DTYPE, VSYN_SEG_RESET, SetupSpec

PAIRS = [(256, 2048), (128, 1024), (512, 4096), (1024, 8192)]
GEOMETRIES = ("beyond2", "beyond_max_a", "beyond_max_b", "short_of_half", "short_of_quarter", "short_of_one", "shared_long",
              "shared_short", "steep")
SHARED = ("shared_long", "shared_short")
MULTS = (1, 2, 3, 4)
RANGE = {1: 256, 2: 128, 3: 86, 4: 64}  # hpp:486-492
DIRECTED = ("ends_top_0", "alternate_0", "single_first", "ends_0_top", "single_last", "ends_top_top", "alternate_1", "single_mid")
RANDOM_ROWS = 4  # per floor, block size and multiplier in floor_cases


# ---- the integer model (hpp:521-589, Utils.hpp:58-183), Python ints only -----------------------------------------------------------

def _low_neighbor(xs, i):
    """Utils.hpp:61-87: among j < i with xs[j] < xs[i], the one with the greatest xs[j]"""
    best = None
    for j in range(i):
        if xs[j] < xs[i] and (best is None or xs[j] > xs[best]):
            best = j
    return best


def _high_neighbor(xs, i):
    """Utils.hpp:92-118: among j < i with xs[j] > xs[i], the one with the smallest xs[j]"""
    best = None
    for j in range(i):
        if xs[j] > xs[i] and (best is None or xs[j] < xs[best]):
            best = j
    return best


def _render_point(x0, y0, x1, y1, X):
    """Utils.hpp:123-137"""
    adx = x1 - x0
    if y1 >= y0:
        return y0 + ((y1 - y0) * (X - x0)) // adx
    return y0 - ((y0 - y1) * (X - x0)) // adx


def unwrap(xs, mult, ys):
    """Step 1, hpp:523-559 -> (final_ys, step2_flag), both in header order. Raises ValueError where the reference fails its CHECK
    (hpp:536) or an amplitude leaves [0, range): no case of this table does."""
    xs = [int(v) for v in xs]
    ys = [int(v) for v in ys]
    rng_of = RANGE[int(mult)]
    n = len(xs)
    flag = [False] * n
    final = [0] * n
    flag[0] = flag[1] = True
    final[0], final[1] = ys[0], ys[1]
    for i in range(2, n):
        lo, hi = _low_neighbor(xs, i), _high_neighbor(xs, i)
        pred = _render_point(xs[lo], final[lo], xs[hi], final[hi], xs[i])
        if not pred <= rng_of:
            raise ValueError("post %d: predicted %d above the range %d" % (i, pred, rng_of))
        val = ys[i]
        high_room, low_room = rng_of - pred, pred
        room = min(high_room, low_room) * 2
        if val == 0:
            final[i] = pred
        else:
            flag[lo] = flag[hi] = flag[i] = True
            if val >= room:
                final[i] = val - low_room + pred if high_room > low_room else pred - val + high_room - 1
            else:
                final[i] = pred - (val + 1) // 2 if val % 2 else pred + val // 2
        if not 0 <= final[i] < rng_of:
            raise ValueError("post %d: amplitude %d outside [0, %d)" % (i, final[i], rng_of))
    return final, flag


def curve(xs, mult, final_ys, flags, n2):
    """Step 2, hpp:563-585, over the n2 bins in use -> uint32[n2]. A segment's values are render_point at every x, which is what
    render_line's DDA walks through (Utils.hpp:144-183; test_oracle_vs_ref.py::test_render_helpers pins the two as equal); a
    segment is cut at n2, and the curve is flat from the last flagged post on."""
    xs = [int(v) for v in xs]
    order = sorted(range(len(xs)), key=lambda i: xs[i])
    out = [0] * n2
    lx, ly = 0, int(final_ys[order[0]]) * int(mult)
    hx = hy = 0
    for i in order[1:]:
        if not flags[i]:
            continue
        hx, hy = xs[i], int(final_ys[i]) * int(mult)
        if lx < n2:
            end = min(hx, n2)
            adx = hx - lx
            if hy >= ly:
                out[lx:end] = [ly + ((hy - ly) * (x - lx)) // adx for x in range(lx, end)]
            else:
                out[lx:end] = [ly - ((ly - hy) * (x - lx)) // adx for x in range(lx, end)]
        lx, ly = hx, hy
    if hx < n2:
        out[hx:n2] = [hy] * (n2 - hx)
    return np.array(out, np.uint32)


# ---- coded rows --------------------------------------------------------------------------------------------------------------------

def encode(xs, mult, target, coded):
    """Coded ys (7.2.3) whose unwrap gives target[i] at every post with coded[i] (by a non-zero code: a target equal to the prediction
    moves by one, towards the middle of the range) and the prediction at every other inner post. Every in-range target has a code."""
    rng_of = RANGE[mult]
    n = len(xs)
    ys = [0] * n
    final = [0] * n
    final[0] = ys[0] = int(target[0])
    final[1] = ys[1] = int(target[1])
    assert 0 <= ys[0] < rng_of and 0 <= ys[1] < rng_of
    for i in range(2, n):
        lo, hi = _low_neighbor(xs, i), _high_neighbor(xs, i)
        pred = _render_point(xs[lo], final[lo], xs[hi], final[hi], xs[i])
        if not coded[i]:
            final[i] = pred
            continue
        t = int(target[i])
        assert 0 <= t < rng_of
        if t == pred:
            t += 1 if pred < rng_of // 2 else -1
        d = t - pred
        hr, lr = rng_of - pred, pred
        room = min(hr, lr) * 2
        if d > 0:
            val = 2 * d if 2 * d < room else d + lr
        else:
            val = -2 * d - 1 if -2 * d - 1 < room else hr - d - 1
        assert 0 < val < 256
        ys[i], final[i] = val, t
    return ys


def directed_rows(xs, mult):
    """-> [(name, ys)] in the order of DIRECTED"""
    top = RANGE[mult] - 1
    n = len(xs)
    order = sorted(range(n), key=lambda i: xs[i])
    inner_sorted = [i for i in order if i >= 2]
    rows = {}
    for name, a, b in (("ends_top_0", top, 0), ("ends_0_top", 0, top), ("ends_top_top", top, top)):
        rows[name] = [a, b] + [0] * (n - 2)
    for phase in (0, 1):
        target = [0] * n
        for s, i in enumerate(order):
            target[i] = top if (s + phase) % 2 else 0
        rows["alternate_%d" % phase] = encode(xs, mult, target, [True] * n)
    for name, pick in (("single_first", 0), ("single_mid", len(inner_sorted) // 2), ("single_last", -1)):
        if not inner_sorted:  # two posts: nothing to code; the ends at mid range instead
            rows[name] = [top // 2, top // 2 + 1]
            continue
        i = inner_sorted[pick]
        ends = [top // 2, top // 2]
        coded = [k == i for k in range(n)]
        at_rest = unwrap(xs, mult, encode(xs, mult, ends + [0] * (n - 2), [False] * n))[0][i]
        target = ends + [0] * (n - 2)
        target[i] = 0 if at_rest > top // 2 else top
        rows[name] = encode(xs, mult, target, coded)
    return [(name, rows[name]) for name in DIRECTED]


def random_row(rng, xs, mult, zero_frac=0.3):
    rng_of = RANGE[mult]
    target = [int(v) for v in rng.integers(0, rng_of, len(xs))]
    coded = [bool(v) for v in rng.random(len(xs)) >= zero_frac]
    return encode(xs, mult, target, coded)


# ---- X lists -----------------------------------------------------------------------------------------------------------------------

def _pick(rng, lo, hi, k):
    assert hi - lo >= k >= 0, (lo, hi, k)
    return [int(v) for v in rng.choice(np.arange(lo, hi), k, replace=False)] if k else []


def _shuffled(rng, inner):
    inner = list(inner)
    rng.shuffle(inner)  # header order is not sorted in real streams
    assert len(set(inner)) == len(inner)
    return [int(v) for v in inner]


def _xs(rng, geom, h, h0, h1):
    if geom == "beyond2":
        posts = int(rng.integers(12, 21))
        beyond = int(rng.integers(3, 6))
        inner = [h - 1, h, h + 1] + _pick(rng, h + 2, 2 * h, beyond) + _pick(rng, 1, h - 1, posts - 5 - beyond)
        return [0, 2 * h] + _shuffled(rng, inner)
    if geom == "beyond_max_a":
        return [0, 32768]
    if geom == "beyond_max_b":
        return [0, 32768] + _shuffled(rng, _pick(rng, 1, h, 9) + _pick(rng, 20000, 32768, 9))
    if geom in ("short_of_half", "short_of_quarter"):
        x1 = h // 2 if geom == "short_of_half" else h // 4
        return [0, x1] + _shuffled(rng, _pick(rng, 1, x1, min(8, x1 - 1)))
    if geom == "short_of_one":
        return [0, 1]
    if geom == "shared_long":
        inner = [h0 - 1, h0, h0 + 1] + _pick(rng, 1, h0 - 1, 4) + _pick(rng, h0 + 2, h1, 8)
        return [0, h1] + _shuffled(rng, inner)
    if geom == "shared_short":
        return [0, h0] + _shuffled(rng, _pick(rng, 1, h0, 9))
    if geom == "steep":
        return [0, h, 1] + _shuffled(rng, [2, 3, h - 3, h - 2, h - 1] + _pick(rng, 4, h - 3, 4))
    raise ValueError(geom)


def floor_lists(geom, bs0, bs1):
    """-> [xs] of the setup's floors: one X list for a shared geometry, else [short, long]"""
    rng = np.random.default_rng([GEOMETRIES.index(geom), bs0, bs1])
    h0, h1 = bs0 // 2, bs1 // 2
    if geom in SHARED:
        return [_xs(rng, geom, h1, h0, h1)]
    return [_xs(rng, geom, h0, h0, h1), _xs(rng, geom, h1, h0, h1)]


def make_spec(geom, bs0, bs1, channels=2, coupled=True):
    """The setup of a geometry: every X list with each multiplier (floor k * 4 + m - 1), one mapping per floor, and modes
    0..3 short / 4..7 long with multiplier 1..4. A shared geometry's modes m - 1 and 4 + m - 1 use the same floor."""
    lists = floor_lists(geom, bs0, bs1)
    floors = [(m, list(xs)) for xs in lists for m in MULTS]
    coup = [(0, 1)] if channels >= 2 and coupled else []
    mappings = [(coup, [f] * channels) for f in range(len(floors))]
    long_base = 0 if geom in SHARED else 4
    modes = [(0, m - 1) for m in MULTS] + [(1, long_base + m - 1) for m in MULTS]
    return SetupSpec(channels, bs0, bs1, floors, mappings, modes)


def mode_floor(spec, mode, c=0):
    """-> (multiplier, xs, block size) of channel c of a mode: the floor spec.floors[spec.mappings[mapping][1][c]] (every channel
    of a mapping uses one floor in this module's setups; multimode_cases.py has mappings whose channels differ)"""
    bf, mp = spec.modes[mode]
    mult, xs = spec.floors[spec.mappings[mp][1][c]]
    return mult, xs, spec.blocksize1 if bf else spec.blocksize0


def floor_cases(geom, bs0, bs1):
    """The (xs, mult, ys, n) rows of a geometry for the floor tail alone (orc_floor1_synth / ref_floor1_synth): per floor, block
    size that uses it and multiplier, the directed rows and RANDOM_ROWS random ones. -> [dict(name, xs, mult, ys, n)]"""
    rng = np.random.default_rng([1000 + GEOMETRIES.index(geom), bs0, bs1])
    lists = floor_lists(geom, bs0, bs1)
    uses = [(lists[0], bs0), (lists[0], bs1)] if geom in SHARED else [(lists[0], bs0), (lists[1], bs1)]
    out = []
    for xs, n in uses:
        for mult in MULTS:
            rows = directed_rows(xs, mult) + [("random_%d" % k, random_row(rng, xs, mult)) for k in range(RANDOM_ROWS)]
            for name, ys in rows:
                out.append(dict(name="%s/%d/x%d/%s" % (geom, n, mult, name), xs=np.array(xs, np.uint32), mult=mult,
                                ys=np.array(ys, np.uint32), n=n))
    return out


# ---- batches -----------------------------------------------------------------------------------------------------------------------

def make_batch(spec, kind, seed=1):
    """A batch on make_spec's setup. kind "mixed": 2 streams (4 when mono) of 24 packets in synth_batch's mixed pattern
    (L L L S*8, rotated per stream); "long": one stream of 24 long packets. Packets of a block size cycle through the multipliers;
    the directed rows of each (block size, multiplier) go to the first rows of that kind, random rows fill the rest. Window flags
    agree with the blocks; residue as synth_batch's (rounded Laplace, 60 % zeros).
    -> dict(packets, segments, ys, residue, plane_stride, rows=[(packet, channel, name)], placed={(long, mult): set of names})"""
    rng = np.random.default_rng([seed, spec.blocksize0, spec.blocksize1, spec.channels, kind == "long"])
    C = spec.channels
    streams, npk = (1, 24) if kind == "long" else (2 if C > 1 else 4, 24)
    unit = [1, 1, 1] + [0] * 8
    flags1 = np.ones(npk, np.uint8) if kind == "long" else np.array((unit * (npk // len(unit) + 1))[:npk], np.uint8)
    queue = {}
    for lng in (0, 1):
        for m in MULTS:
            mult, xs, _ = mode_floor(spec, 4 * lng + m - 1)
            queue[(lng, m)] = directed_rows(xs, mult)
    placed = {k: set() for k in queue}
    count = [0, 0]
    P = streams * npk
    pk = np.zeros(P, PACKET_DTYPE)
    seg = np.zeros(streams, SEGMENT_DTYPE)
    ys = np.zeros((P, C, spec.ys_stride), np.uint16)
    rows, res_parts = [], []
    off = 0
    for s in range(streams):
        flags = flags1 if kind == "long" else np.roll(flags1, s % 11)
        seg[s] = (s, s * npk, npk, VSYN_SEG_RESET, off)
        for q in range(npk):
            p = s * npk + q
            lng = int(flags[q])
            m = MULTS[count[lng] % 4]
            count[lng] += 1
            mode = 4 * lng + m - 1
            mult, xs, n = mode_floor(spec, mode)
            pk[p]["mode"] = mode
            if lng:
                pk[p]["prev_long"] = flags[q - 1] if q > 0 else 1
                pk[p]["next_long"] = flags[q + 1] if q + 1 < npk else 1
            pk[p]["granule"] = -1
            pk[p]["floor_used"] = (1 << C) - 1
            for c in range(C):
                if queue[(lng, m)]:
                    name, row = queue[(lng, m)].pop(0)
                    placed[(lng, m)].add(name)
                else:
                    name, row = "random", random_row(rng, xs, mult)
                ys[p, c, :len(xs)] = row
                rows.append((p, c, name))
            r = np.round(rng.laplace(0.0, 1.5, (C, n // 2)))
            r[rng.random((C, n // 2)) < 0.6] = 0
            res_parts.append(r.astype(np.float32).ravel())
            off += C * (n // 2)
    return dict(packets=pk, segments=seg, ys=ys, residue=np.concatenate(res_parts), plane_stride=npk * (spec.blocksize1 // 2) + 64,
                rows=rows, placed=placed)


def model_taps(spec, b):
    """The integer model's floor_final [P * C * ys_stride] and floor_curve [residue.size] of a batch, in the layout of the
    vsyn_taps of the same names: final_y * multiplier | step2_flag << 15 per post; the curve per bin, packed like the residue.
    Every row takes the floor of its own channel; a channel whose floor_used bit is clear leaves both taps at zero."""
    from tests.workloads import packet_blocks
    C, stride = spec.channels, spec.ys_stride
    n_of, off = packet_blocks(spec, b["packets"], b["segments"])
    final = np.zeros((len(b["packets"]), C, stride), np.uint16)
    crv = np.zeros(b["residue"].size, np.uint16)
    memo = {}
    for p in range(len(b["packets"])):
        mode = int(b["packets"]["mode"][p])
        used = int(b["packets"]["floor_used"][p])
        for c in range(C):
            mult, xs, n = mode_floor(spec, mode, c)
            assert n == n_of[p]
            if not (used >> c) & 1:
                continue
            row = tuple(int(v) for v in b["ys"][p, c, :len(xs)])
            key = (spec.mappings[spec.modes[mode][1]][1][c], n, row)
            if key not in memo:
                fy, fl = unwrap(xs, mult, row)
                memo[key] = (np.array([v * mult | (int(f) << 15) for v, f in zip(fy, fl)], np.uint16), curve(xs, mult, fy, fl, n // 2))
            final[p, c, :len(xs)] = memo[key][0]
            crv[off[p] + c * (n // 2): off[p] + (c + 1) * (n // 2)] = memo[key][1]
    return final.ravel(), crv
