"""The case table of tests/resample_cases.py keeps its promises, on the CPU: every case reaches the kernel variant, the chunks, the
edge and the 2^32 crossing it names, by a restatement of the host plan whose constants are read from csrc/vsyn_resample.h; the span
bound rs_span4 is never exceeded over a full period of tile starts and is reached where the table says; and the checks that
tests/test_gpu_resample_shapes.py applies to the device hold on the float64 model and on a float32 multiply-add chain. Last, the
kernel's tile loop restated in numpy passes those checks as written and fails them with a 32-bit tile position, a span bound one
float4 short or chunk-local output indices: the breaks are tried there, not on a device."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
from parseoggvorbis_amd import binding
from tests import resample_cases as rc
from tests import resample_model as rm

PAIRS = sorted({(r, c["out_rate"]) for c in rc.CASES for r in c["in_rates"] if r})
SMALL = [(44100, 16000, 700), (16000, 44100, 300), (22050, 16000, 1500), (380, 31, 9000), (204, 13, 9000), (37084, 44100, 200),
         (65536, 65535, 60), (65521, 65536, 5), (1, 65536, 2), (65536, 1, 70000)]


def test_the_restated_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parseoggvorbis_amd", "csrc", "vsyn_resample.h")).read()
    define = lambda name: re.search(r"#define\s+%s\s+(.+?)\s*(?://.*)?$" % name, src, re.M).group(1)  # noqa: E731
    assert (int(define("RS_THREADS")), int(define("RS_PER_THREAD")), int(define("RS_TILES"))) == (rc.RS_THREADS, rc.RS_PER_THREAD, rc.RS_TILES)
    assert define("RS_TILE") == "(RS_THREADS * RS_PER_THREAD)" and define("RS_CHUNK") == "(RS_TILE * RS_TILES)"
    kib = re.search(r"static const uint32_t RS_LDS_BUDGET = (\d+)u \* 1024u;", src)
    assert kib and int(kib.group(1)) * 1024 == rc.RS_LDS_BUDGET
    # the formulas the restatement restates, as the header has them
    for line in ("const uint64_t d = ((uint64_t)(RS_TILE - 1) * down + up - 1u) / up;", "return (uint32_t)((d + k4 + 3u) / 4u + 1u);",
                 "const uint64_t lds = 4ull * ((uint64_t)p.up * p.k4 + 4ull * p.span4);", "p.lds = lds <= RS_LDS_BUDGET;",
                 "p.k4 = (K + 3u) & ~3u;", "const uint64_t c0 = j0 * down + pr.h;", "a0 = ((int64_t)qb - (int64_t)(k4 - 1u)) & ~(int64_t)3;",
                 "const uint32_t m4 = min((uint32_t)((e - a0) / 4 + 1), pr.span4);", "(int)RS_LDS_BUDGET));"):
        assert line in src, line


@pytest.mark.parametrize("case", rc.CASES, ids=rc.IDS)
def test_case_reaches_what_it_states(case):
    assert rc.reach(case) == case["reach"]
    assert all(rm.valid(r, case["out_rate"]) for r in case["in_rates"] if r)
    assert 1 <= case["channels"] <= 255 and len({c["name"] for c in rc.CASES}) == len(rc.CASES)


def test_the_table_has_the_cases():
    """Each thing the table is there for, by name."""
    R = {c["name"]: c["reach"] for c in rc.CASES}
    B = rc.BY_NAME
    # 64-bit positions: tiles past 2^32 exist in both variants, with outputs behind the crossing
    assert R["long_lds"]["past32"] == {44100: 9511} and 9511 * rc.RS_TILE == 9_739_264 < rc.seg_out_frames(B["long_lds"], 0)
    assert R["long_global"]["past32"] == {65536: 64} and R["long_global"]["pairs"][65536][0] == "global"
    a, n = B["long_lds"]["stretch"]
    lo, hi = rc.footprint(44100, 16000, 27_000_000, a, a + n)
    assert 9511 * rc.RS_TILE < lo < hi < rc.seg_out_frames(B["long_lds"], 0)
    for q in rc.impulse_planes(B["long_lds"], 0)[0]:  # the impulses and the stretch share no output
        assert q + 56 <= a or q >= a + n + 56
    # the contract's limit, both ways, and a prime
    assert {rm.ratio(r, c["out_rate"]) for c in rc.CASES for r in c["in_rates"] if r} >= {(1, 65536), (65536, 1), (65536, 65535), (65536, 65521),
                                                                                         (65535, 65536)}
    assert B["down_65536"]["frames"][2] == 3 and B["up_65536_from_1"]["frames"][0] == 3
    # the budget: equality is the LDS variant, 16 bytes more is not
    assert rc.plan(380, 31)["lds_bytes"] == rc.RS_LDS_BUDGET and rc.plan(380, 31)["variant"] == "lds"
    assert rc.plan(204, 13)["lds_bytes"] == rc.RS_LDS_BUDGET + 16 and rc.plan(204, 13)["variant"] == "global"
    for name in ("budget_lds", "budget_global"):
        To = [rc.seg_out_frames(B[name], g) for g in range(2)]
        assert 2 * rc.RS_TILE < To[0] < rc.RS_CHUNK and To[1] > 2 * rc.RS_CHUNK
    # every edge length, per variant; three chunks of the global variant and of the copy
    e = B["edges"]
    for r in (44100, 44056, 16000):
        assert tuple(rc.seg_out_frames(e, g) for g in range(len(e["frames"])) if e["in_rates"][g] == r) == rc.EDGES
    assert R["edges"]["chunks"] == {"lds": 3, "global": 3, "copy": 3}
    # the widest span of 22050 -> 16000: tile 4, which 7000 frames do not fill and 7056 do
    assert R["widest_span"]["widest"] == {22050: 4} and rc.first_widest_tile(rc.plan(22050, 16000), rm.num_frames(22050, 16000, 7000)) is None
    assert 7000 < rc.frames_for(22050, 16000, 5 * rc.RS_TILE) <= 7056 == min(B["widest_span"]["frames"])
    assert R["pitch_pair"]["chunks"] == {"global": 3} and rm.ratio(37084, 44100) == (11025, 9271)
    # alignment: three plane strides by four input offsets, every output offset, one run aligned throughout
    al = [c for c in rc.CASES if c["name"].startswith("align_")]
    assert {(c["plane"] % 4, c["in_off"]) for c in al} == {(s, o) for s in (0, 1, 2) for o in range(4)}
    assert {c["out_off"] for c in al} == {0, 1, 2, 3} and {(c["plane"] + c["out_pad"]) % 4 for c in al} <= {0, 1, 2, 3}
    assert (B[rc.ALIGNED]["plane"] % 4, B[rc.ALIGNED]["in_off"], B[rc.ALIGNED]["out_off"], rc.out_plane(B[rc.ALIGNED]) % 4) == (0, 0, 0, 1)
    assert all(c["channels"] == 2 and c["frames"] == B[rc.ALIGNED]["frames"] for c in al)
    # many segments: more than two passes of the 256-thread scan, every frame count under every rate, runs of equal offsets
    m = B["many_segments"]
    assert len(m["frames"]) == 700 and {(r, f) for r, f in zip(m["in_rates"], m["frames"])} == {(r, f) for r in (44100, 44056, 16000, 0)
                                                                                                for f in (0, 1, 5, 300, 9000)}
    assert B["frames_past_plane"]["frames"] == [B["frames_past_plane"]["plane"] + 1000] * 3 and B["channels_255"]["channels"] == 255


@pytest.mark.parametrize("r_in,r_out", PAIRS, ids=["%d_%d" % p for p in PAIRS])
def test_span_bound_over_a_full_period(r_in, r_out):
    """rs_span4 against the span the kernel computes, over every tile start of a period, full tiles and every shorter last tile
    length that matters (a shorter tile reads no further): never exceeded; reached exactly by the LDS pairs of the table."""
    p = rc.plan(r_in, r_out)
    if p["variant"] == "copy":
        return
    tiles = np.arange(rc.span_period(p), dtype=np.int64)
    m4 = rc.tile_span4(p, tiles)
    assert m4.max() <= p["span4"], (r_in, r_out, int(m4.max()), p["span4"])
    assert (rc.tile_span4(p, tiles, kn=1) <= m4).all()
    assert np.array_equal(rc.tile_span4(p, tiles + rc.span_period(p)), m4)  # it is a period
    if p["variant"] == "lds":
        assert m4.max() == p["span4"]
        assert 16 * p["span4"] + p["table_bytes"] == p["lds_bytes"] <= rc.RS_LDS_BUDGET
        # the staged span holds every input the tile's outputs read: first tap of the first output, i0 of the last
        c0 = tiles * rc.RS_TILE * p["down"] + p["H"]
        a0 = (c0 // p["up"] - (p["K4"] - 1)) & ~np.int64(3)
        last = rc.i0_of(p, tiles * rc.RS_TILE + rc.RS_TILE - 1)
        assert (a0 <= c0 // p["up"] - (p["K4"] - 1)).all() and (last < a0 + 4 * m4).all()


@pytest.mark.parametrize("r_in,r_out,T", SMALL, ids=["%d_%d" % s[:2] for s in SMALL])
def test_resample_at_and_the_impulse_identity_on_the_model(r_in, r_out, T):
    """resample_at is resample at those indices, bit for bit; and for a unit impulse at p, resample(delta_p)[j] is the tap
    h[tap_index(j, p)], and 0 where there is none: check_impulses holds on the model."""
    rng = np.random.default_rng(T)
    x = rng.uniform(-1.0, 1.0, (2, T)).astype(np.float32)
    full = rm.resample(x, r_in, r_out)
    To = full.shape[1]
    assert To == rm.num_frames(r_in, r_out, T)
    j = np.unique(np.concatenate([[0, To - 1], rng.integers(0, To, 50)]))
    assert np.array_equal(rm.resample_at(x, r_in, r_out, j), full[:, j])
    assert np.array_equal(rm.resample_at(x[0], r_in, r_out, j, block=1000), full[0, j])
    assert np.array_equal(rm.resample_at(x[1], r_in, r_out, np.arange(To)), full[1])
    h, P = rc.tables(r_in, r_out)
    K4 = P.shape[1]
    for p in sorted({0, T - 1, T // 2, min(T - 1, K4)}):
        d = np.zeros(T, np.float32)
        d[p] = 1.0
        y = rm.resample(d, r_in, r_out)
        n = rm.tap_index(r_in, r_out, np.arange(To), p)
        assert np.array_equal(y, np.where(n >= 0, h[np.maximum(n, 0)], 0.0)), p
        assert rc.check_impulses(y.astype(np.float32), r_in, r_out, T, [p], (r_in, r_out, p)) <= 0.5  # float32 of the same double
        lo, hi = rc.footprint(r_in, r_out, T, p, p + 1)
        assert not y[:lo].any() and not y[hi:].any()
        assert hi > lo and n[lo] >= 0 and (n[lo:hi] >= 0).sum() == (n >= 0).sum()  # the footprint begins at the first output with a tap
    # a tap moved by one input or by one output is caught
    d = np.zeros(T, np.float32)
    d[T // 2] = 1.0
    with pytest.raises(AssertionError):
        rc.check_impulses(np.roll(rm.resample(d, r_in, r_out), 1).astype(np.float32), r_in, r_out, T, [T // 2], "rolled")
    if T > 3:
        with pytest.raises(AssertionError):
            rc.check_impulses(rm.resample(d, r_in, r_out).astype(np.float32), r_in, r_out, T, [T // 2 - 1], "moved")


def test_tap_index_by_hand():
    # 2 -> 1: up 1, down 2, H = 20, N = 41: output j reads x[2 j + 20 - t] with tap h[t]; sample 100 is tap 2 j - 80, for j 40 .. 60
    n = rm.tap_index(2, 1, np.arange(70), 100)
    assert n[40:61].tolist() == list(range(0, 41, 2)) and (n[:40] == -1).all() and (n[61:] == -1).all()
    # 1 -> 2: up 2, down 1, H = 20, N = 41: c = j + 20, phi = c % 2, i0 = c // 2; sample 3: n = phi + (i0 - 3) 2 = j + 14
    n = rm.tap_index(1, 2, np.arange(40), 3)
    assert n[:27].tolist() == list(range(14, 41)) and (n[27:] == -1).all()


@pytest.mark.parametrize("r_in,r_out", [p for p in PAIRS if p not in ((65536, 1), (16000, 16000))], ids=lambda v: str(v))
def test_model_matches_scipy_on_the_new_pairs(r_in, r_out):
    """As tests/test_resample_cpu.py, on the table's pairs (65536 -> 1 would take scipy an hour-long filter design for 4 outputs;
    its taps are the same formula at M = 65536 that 1 -> 65536 checks)."""
    signal = pytest.importorskip("scipy.signal")
    up, down = rm.ratio(r_in, r_out)
    rng = np.random.default_rng(r_in + r_out)
    for T in ((3, 40) if up == 65536 else (3, 40, 3000)):
        x = rng.uniform(-1.0, 1.0, T).astype(np.float32)
        got = rm.resample(x, r_in, r_out)
        want = signal.resample_poly(x, up, down)
        assert want.shape == got.shape
        assert np.abs(got - want).max() <= 1e-6 * max(1, -(-down // up) // 8), (T, np.abs(got - want).max())


def _chain32(x, r_in, r_out, j):
    """y[j] by a float32 multiply-add chain, t ascending, two roundings per term (the product, then the sum), float32 taps."""
    p = rc.plan(r_in, r_out)
    P = rc.tables(r_in, r_out)[1].astype(np.float32)
    T = x.shape[0]
    out = np.zeros(j.size, np.float32)
    t = np.arange(p["K4"])[None, :]
    rows = max(1, (1 << 22) // p["K4"])
    for a in range(0, j.size, rows):
        c = j[a:a + rows] * p["down"] + p["H"]
        idx = (c // p["up"])[:, None] - t
        v = np.where((idx >= 0) & (idx < T), x[np.clip(idx, 0, T - 1)], np.float32(0))
        out[a:a + rows] = np.cumsum(P[c % p["up"]] * v, axis=1, dtype=np.float32)[:, -1]
    return out


@pytest.mark.parametrize("name", ["budget_lds", "budget_global", "down_65536", "long_global", "widest_span"])
def test_the_chain_bound_holds_for_a_float32_chain(name):
    """B_j (resample_cases.bound) on the case's own noise: a float32 chain that rounds twice per term, which is no better than the
    device's fused chain, stays inside it at every output tried, and for the long chains far inside it."""
    case = rc.BY_NAME[name]
    x = rc.noise_input(case)
    worst = 0.0
    for g, r in enumerate(case["in_rates"]):
        T, To = rc.seg_frames(case, g), rc.seg_out_frames(case, g)
        j = np.unique(np.linspace(0, To - 1, min(To, 1500)).astype(np.int64))
        xs = x[g, 0, :T]
        d = np.abs(_chain32(xs, r, case["out_rate"], j).astype(np.float64) - rm.resample_at(xs, r, case["out_rate"], j, P=rc.tables(r, case["out_rate"])[1]))
        B = rc.bound(xs, r, case["out_rate"], j)
        assert (B > 0).all()
        worst = max(worst, float((d / B).max()))
    print("%s: float32 chain at %.3g of B_j" % (name, worst))
    assert worst <= 1.0
    if rc.plan(case["in_rates"][0], case["out_rate"])["K4"] > 100000:
        assert worst <= 1e-3


def test_inputs_are_seeded_and_impulses_stand_apart():
    for case in rc.CASES:
        if case["name"] in ("long_lds", "many_segments") or (case["name"].startswith("align_") and case["name"] != rc.ALIGNED):  # big, or repeats
            continue
        a, b = rc.impulse_input(case), rc.impulse_input(case)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        for g, r in enumerate(case["in_rates"]):
            T = rc.seg_frames(case, g)
            planes = rc.impulse_planes(case, g)
            assert np.isnan(a[g, :, T:]).all() and np.isfinite(a[g, :, :T]).all()
            if not r or not T:
                continue
            got = sorted(q for pl in planes for q in pl)
            assert 0 in got and (T - 1 in got or T == 1), (case["name"], g)
            if rc.plan(r, case["out_rate"])["variant"] != "copy":
                for c, pl in enumerate(planes):
                    assert np.flatnonzero(a[g, c, :T]).tolist() == sorted(pl)
                    rc.impulse_outputs(r, case["out_rate"], T, pl)  # asserts that no output sees two


def test_num_frames_of_the_library_on_the_table():
    entry.build_hip()
    f = binding.load().vsyn_resample_num_frames
    for case in rc.CASES:
        for g, r in enumerate(case["in_rates"]):
            if r:
                up, down = rm.ratio(r, case["out_rate"])
                for T in (case["frames"][g], rc.seg_frames(case, g), case["plane"], 2 ** 32 - 1):
                    assert f(r, case["out_rate"], T) == -(-T * up // down) == rm.num_frames(r, case["out_rate"], T)
    for r_in, To in ((44100, e) for e in rc.EDGES):
        T = rc.frames_for(r_in, 16000, To)
        assert f(r_in, 16000, T) == To and f(r_in, 16000, T - 1) == To - 1


def _emulate(x, r_in, r_out, tiles, lds=True, c0_bits=64, span_short=0, chunk_local=False):
    """vsyn_rs_kernel's tile loop restated for some tiles of one plane x [T], with the breaks the device module is built to catch as
    switches: the tile position kept in c0_bits bits, the staged span span_short float4s short of rs_span4, the output index taken
    from the chunk's start. Float32 taps, float64 sums. The span image persists from tile to tile as the LDS does (NaN before the
    first tile: anything may be there). Returns {j: y[j]} arrays (j, y) over the tiles' outputs."""
    p = rc.plan(r_in, r_out)
    P = rc.tables(r_in, r_out)[1].astype(np.float32).astype(np.float64)
    T, To = x.shape[0], rm.num_frames(r_in, r_out, x.shape[0])
    up, down, K4 = p["up"], p["down"], p["K4"]
    sX = np.full(4 * p["span4"] + 8, np.nan)
    js, ys = [], []
    for tile in tiles:
        j0 = tile * rc.RS_TILE
        kn = min(rc.RS_TILE, To - j0)
        c0 = (j0 * down + p["H"]) & (2 ** c0_bits - 1)
        qb, rb = c0 // up, c0 % up
        k = np.arange(kn, dtype=np.int64)
        cr = rb + k * down
        phi, i0 = cr % up, qb + cr // up
        idx = i0[:, None] - np.arange(K4)[None, :]
        if lds:
            a0 = (qb - (K4 - 1)) & ~3
            m4 = min((qb + (rb + (kn - 1) * down) // up - a0) // 4 + 1, p["span4"] - span_short)
            i = a0 + np.arange(4 * m4, dtype=np.int64)
            sX[:4 * m4] = np.where((i >= 0) & (i < T), x[np.clip(i, 0, T - 1)], 0.0)
            v = sX[idx - a0]
        else:
            v = np.where((idx >= 0) & (idx < T), x[np.clip(idx, 0, T - 1)], 0.0)
        js.append((j0 % rc.RS_CHUNK if chunk_local else j0) + k)
        ys.append((P[phi] * v).sum(axis=1))
    return np.concatenate(js), np.concatenate(ys).astype(np.float32)


def _emulated_plane(case, cls, tiles=None, **breaks):
    """The first plane of the case's first segment as the emulation gives it (outside `tiles`: what is expected there), checked as the device's is:
    raises AssertionError where the device module would fail."""
    r, out = case["in_rates"][0], case["out_rate"]
    T, To = rc.seg_frames(case, 0), rc.seg_out_frames(case, 0)
    x = (rc.impulse_input(case) if cls == "impulses" else rc.noise_input(case))[0, 0, :T]
    every = tiles is None
    tiles = range(-(-To // rc.RS_TILE)) if every else tiles
    j, yj = _emulate(x, r, out, tiles, lds=rc.plan(r, out)["variant"] == "lds", **breaks)
    y = np.zeros(To, np.float32)
    if cls == "impulses" and not every:  # outside the emulated tiles: what is expected there
        je, we = rc.impulse_outputs(r, out, T, rc.impulse_planes(case, 0)[0])
        y[je] = we
    y[j] = yj
    if cls == "impulses":
        skip = rc.footprint(r, out, T, case["stretch"][0], sum(case["stretch"])) if case["stretch"] else None
        rc.check_impulses(y, r, out, T, rc.impulse_planes(case, 0)[0], case["name"], skip)
        if skip:
            jj = np.sort(j[(j >= skip[0]) & (j < skip[1])])
            assert jj.size
            rc.check_noise(y[jj], x, r, out, case["name"], j=jj)
    else:
        jj = np.arange(To) if every else np.sort(j)
        rc.check_noise(y[jj], x, r, out, case["name"], j=jj)


BREAKS = [("long_lds", "impulses", dict(c0_bits=32)), ("long_global", "impulses", dict(c0_bits=32)), ("long_global", "noise", dict(c0_bits=32)),
          ("widest_span", "impulses", dict(span_short=1)), ("widest_span", "noise", dict(span_short=1)), ("budget_lds", "impulses", dict(span_short=1)),
          ("budget_lds", "noise", dict(span_short=1)), ("edges", "noise", dict(chunk_local=True)), ("pitch_pair", "impulses", dict(chunk_local=True))]


@pytest.mark.parametrize("name,cls,breaks", BREAKS, ids=["%s-%s-%s" % (n, c, "_".join(b)) for n, c, b in BREAKS])
def test_the_checks_catch_the_breaks_on_an_emulated_kernel(name, cls, breaks):
    """No break is tried on the device here: the kernel's tile loop is restated in numpy with each break as a switch. As written it
    passes the very checks the device module applies; with a 32-bit tile position (long_lds, long_global: the tiles past 2^32), a
    span one float4 short (widest_span: tile 4; budget_lds) or chunk-local output indices it fails them."""
    case = rc.BY_NAME[name]
    if name == "edges":  # its longest LDS segment: T_out = 16385, three chunks
        case = dict(case, in_rates=case["in_rates"][7:8], frames=case["frames"][7:8])
    tiles = None
    if name == "long_lds":  # the tiles behind the crossing: the first two, three under the noise, the last two
        lo, _ = rc.footprint(44100, 16000, case["plane"], case["stretch"][0], sum(case["stretch"]))
        last = (rc.seg_out_frames(case, 0) - 1) // rc.RS_TILE
        tiles = [9511, 9512] + [lo // rc.RS_TILE + k for k in (1, 2, 3)] + [last - 1, last]
    _emulated_plane(case, cls, tiles)
    with pytest.raises(AssertionError):
        _emulated_plane(case, cls, tiles, **breaks)
