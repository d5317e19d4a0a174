"""Pins the CPU oracle (oracle/vorbis_synth_oracle.c) against the REFERENCE ITSELF: the answers of the reference's own
code (oracle/_ref/libref_shim.so, built from its sources by oracle/Makefile) on the seeded inputs below are stored in
tests/golden/ref_shim.npz by oracle/make_ref_vectors.py, so the suite needs no reference tree.
Bit-exact for everything: same arithmetic, same order.  Large outputs are stored as the sha256 of their bits.
"""
import hashlib
import os

import numpy as np
import pytest

from oracle import oracle_binding as ob
from tests import floor_geometry_cases as fg

SIZES = [64, 128, 256, 512, 1024, 2048, 4096, 8192]  # every Vorbis I blocksize, hpp:1294
CLOSED_FORM_SIZES = [64, 256, 2048]
WINDOW_PAIRS = [(256, 2048), (64, 64), (64, 8192), (512, 1024), (2048, 2048)]
WINDOW_CASES = [(flag, prev, nxt) for flag in (0, 1) for prev in (0, 1) for nxt in (0, 1)]
FLOOR_MULTS = [1, 2, 3, 4]
FLOOR_SHAPES = [(2, 64), (9, 256), (29, 2048), (65, 8192), (17, 128)]
FLOOR_TRIALS = 25
OVERLAP_CONFIGS = [(256, 2048, 2), (64, 128, 1), (128, 128, 3), (64, 8192, 2)]
OVERLAP_TRIALS = 4
# window flags that disagree with the block sequence (classes of tests/README.md): block-size pairs, channels
WINFLAG_CONFIGS = [(256, 2048, 2), (64, 8192, 1), (4096, 8192, 1), (128, 1024, 2), (512, 4096, 1), (1024, 2048, 1), (256, 256, 2)]
WINFLAG_TRIALS = ("bcd", "bcd_granule", "a", "random")

REF_VECTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_shim.npz")
_vectors = None


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def digest(a):
    """sha256 of an array's dtype, shape and bytes: equal digests <=> equal arrays, bit for bit."""
    a = np.ascontiguousarray(a)
    h = hashlib.sha256()
    h.update(("%s %s " % (a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def ref_vector(key):
    global _vectors
    if _vectors is None:
        _vectors = np.load(REF_VECTORS)
    return _vectors[key]


def assert_ref(key, got):
    """got == the reference's answer stored under key (the array itself, or the digest of its bits)."""
    want = ref_vector(key)
    if want.dtype.kind == "U":
        assert digest(got) == str(want), key
    else:
        assert got.dtype == want.dtype and np.array_equal(got, want), key


# ---- seeded inputs (shared with oracle/make_ref_vectors.py, which stores the reference's answers to them) ----

def mdct_input(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((16, n // 2)).astype(np.float32)
    x[0] = 0
    x[1, :] = 0
    x[1, 3] = 1.0  # impulse
    return x


def closed_form_input(n):
    rng = np.random.default_rng(7)
    return (rng.standard_normal(n // 2) * 0.05).astype(np.float32)


def render_inputs():
    """-> (render_point args [2000 x 5], render_line (x0, y0, x1, y1, len) [300], neighbor sets [200])"""
    rng = np.random.default_rng(3)
    points = []
    for _ in range(2000):
        x0 = int(rng.integers(0, 1000))
        x1 = x0 + int(rng.integers(1, 600))
        y0, y1 = int(rng.integers(0, 256)), int(rng.integers(0, 256))
        X = int(rng.integers(x0, x1 + 1))
        points.append((x0, y0, x1, y1, X))
    lines = []
    for _ in range(300):
        ln = int(rng.integers(8, 1200))
        x0 = int(rng.integers(0, ln + 20))
        x1 = x0 + int(rng.integers(1, 700))
        y0, y1 = int(rng.integers(0, 256)), int(rng.integers(0, 256))
        lines.append((x0, y0, x1, y1, ln))
    sets = []
    for _ in range(200):
        k = int(rng.integers(3, 66))
        sets.append(rng.permutation(5000)[:k].astype(np.uint32))
    return np.array(points, np.uint32), lines, sets


def random_xs(rng, posts, n2):
    inner = rng.choice(np.arange(1, n2), size=posts - 2, replace=False)
    return np.concatenate([[0, n2], inner]).astype(np.uint32)


def valid_ys(rng, xs, mult, zero_frac=0.3):
    """Random coded ys that decode to in-range amplitudes (what an encoder would produce)."""
    rng_of = {1: 256, 2: 128, 3: 86, 4: 64}[mult]
    posts = len(xs)
    ys = np.zeros(posts, np.uint32)
    fy = np.zeros(posts, np.int64)
    orc = ob.oracle()
    ys[0], ys[1] = rng.integers(0, rng_of, 2)
    fy[0], fy[1] = ys[0], ys[1]
    for i in range(2, posts):
        lo, hi = orc.orc_low_neighbor(ob.p(xs), i), orc.orc_high_neighbor(ob.p(xs), i)
        pred = orc.orc_render_point(int(xs[lo]), int(fy[lo]), int(xs[hi]), int(fy[hi]), int(xs[i]))
        if rng.random() < zero_frac:
            ys[i], fy[i] = 0, pred
            continue
        target = int(rng.integers(0, rng_of))
        hr, lr = rng_of - pred, pred
        room = min(hr, lr) * 2
        d = target - pred
        if d == 0:
            ys[i], fy[i] = 0, pred
            continue
        if d > 0:
            val = d * 2 if d * 2 < room else d + lr  # even branch / overflow-high branch
            if not (d * 2 < room) and not (hr > lr):
                val = 0
        else:
            val = -d * 2 - 1 if -d * 2 - 1 < room else hr - d - 1
            if not (-d * 2 - 1 < room) and (hr > lr):
                val = 0
        ys[i] = val
        if val == 0:
            fy[i] = pred
        elif val >= room:
            fy[i] = val - lr + pred if hr > lr else pred - val + hr - 1
        else:
            fy[i] = pred - (val + 1) // 2 if val % 2 else pred + val // 2
        if not (0 <= fy[i] < rng_of) or val > 255:
            ys[i], fy[i] = 0, pred
    return ys


def floor1_inputs(mult, posts, n):
    """-> [(xs, ys)] of the trials"""
    rng = np.random.default_rng(1000 * mult + posts)
    out = []
    for trial in range(FLOOR_TRIALS):
        xs = random_xs(rng, posts, n // 2)
        ys = valid_ys(rng, xs, mult) if trial % 5 else rng.integers(0, 60, posts).astype(np.uint32)  # some wild ones
        out.append((xs, ys))
    return out


def make_seq(rng, npk):
    """Block-flag sequence with consistent prev/next window flags."""
    flags = rng.integers(0, 2, npk).astype(np.uint8)
    widx = np.zeros(npk, np.uint8)
    for i in range(npk):
        if flags[i]:
            prev = flags[i - 1] if i > 0 else rng.integers(0, 2)
            nxt = flags[i + 1] if i + 1 < npk else rng.integers(0, 2)
            widx[i] = int(prev) | (int(nxt) << 1)
    return flags, widx


def overlap_inputs(bs0, bs1, channels):
    """-> [dict(flags, widx, sizes, blocks, gran, cap)] of the trials: random mixed block sequences with a clipping granule on
    the last packet of every other trial"""
    rng = np.random.default_rng(bs0 + bs1 + channels)
    out = []
    for trial in range(OVERLAP_TRIALS):
        npk = int(rng.integers(2, 40))
        flags, widx = make_seq(rng, npk)
        sizes = np.where(flags, bs1, bs0)
        blocks = [rng.standard_normal((channels, int(s))).astype(np.float32) for s in sizes]
        total = sum(int(sizes[i - 1]) // 4 + int(sizes[i]) // 4 for i in range(1, npk))
        gran = np.full(npk, -1, np.int64)
        if trial % 2:
            gran[-1] = max(0, total - int(rng.integers(0, min(sizes[-1], sizes[-2]) // 4)))
        out.append(dict(flags=flags, widx=widx, sizes=sizes, blocks=blocks, gran=gran, cap=total + 16))
    return out


def winflag_seq(rng, npk, allow_a):
    """Block flags in random stretches, and window flags drawn at random for every block instead of from its neighbours. The four
    ways a long block's flags can disagree with the blocks around it:
      A  long block with next_long set, then a smaller block     (the reference keeps the long right slope past the smaller block)
      B  short block, then a long block with prev_long set
      C  long block with next_long clear, then a long block
      D  long block, then a long block with prev_long clear
    Each of B, C, D is forced at least once; A occurs (forced at least three times) only if allow_a. Short blocks get random flag
    bits too, which the window choice must ignore."""
    flags = np.zeros(npk, np.uint8)
    q = 0
    while q < npk:
        k = int(rng.integers(1, 7))
        flags[q:q + k] = 1
        q += k + int(rng.integers(1, 6))
    flags[:4] = (1, 1, 0, 1)  # long long short long: C or D at 0/1, B or A around 2
    flags[4:8] = (1, 1, 1, 0)
    widx = rng.integers(0, 4, npk).astype(np.uint8)
    nxt_short = np.concatenate([flags[1:] == 0, [False]])
    if not allow_a:
        widx[(flags == 1) & nxt_short] &= 1
    # forced classes: B at 3 (short 2 in front), D at 1 (long 0 in front), C at 4 (long 5 behind)
    widx[3] |= 1
    widx[1] &= 2
    widx[4] &= 1
    if allow_a:
        longs_before_short = np.flatnonzero((flags == 1) & nxt_short)
        for i in list(longs_before_short[:2]) + list(longs_before_short[-1:]):  # early (slides to come) and late
            widx[i] |= 2
    return flags, widx


def has_class_a(flags, widx, bs0, bs1):
    return bs0 < bs1 and bool(((flags[:-1] == 1) & ((widx[:-1] & 2) != 0) & (flags[1:] == 0)).any())


def winflag_inputs(bs0, bs1, channels):
    """-> [dict(flags, widx, sizes, blocks, gran, cap)] of the WINFLAG_TRIALS: sequences of >= 200 packets, so that the reference's
    buffer (5 bs0 + 5 bs1 floats) slides many times, left and right"""
    rng = np.random.default_rng(7 * bs0 + bs1 + channels)
    out = []
    for kind in WINFLAG_TRIALS:
        npk = int(rng.integers(200, 260))
        flags, widx = winflag_seq(rng, npk, allow_a=kind in ("a", "random"))
        if kind == "random":
            widx = rng.integers(0, 4, npk).astype(np.uint8)
        sizes = np.where(flags, bs1, bs0)
        blocks = [rng.standard_normal((channels, int(s))).astype(np.float32) for s in sizes]
        total = sum(int(sizes[i - 1]) // 4 + int(sizes[i]) // 4 for i in range(1, npk))
        gran = np.full(npk, -1, np.int64)
        if kind == "bcd_granule":
            gran[-1] = max(0, total - int(rng.integers(0, min(sizes[-1], sizes[-2]) // 4)))
        out.append(dict(kind=kind, flags=flags, widx=widx, sizes=sizes, blocks=blocks, gran=gran, cap=total + 16))
    return out


def overlap_ref_call(lib, fn, bs0, bs1, channels, c):
    """ref_overlap_add / orc_overlap_add on one trial -> (rc, emit_len, pcm [channels][cap])"""
    import ctypes
    npk, cap = len(c["flags"]), c["cap"]
    pcm = np.zeros((channels, cap), np.float32)
    emit = np.zeros(npk, np.uint32)
    bad = ctypes.c_int(-1)
    flat = np.concatenate([b.ravel() for b in c["blocks"]])
    rc = getattr(lib, fn)(channels, bs0, bs1, npk, ob.p(c["flags"]), ob.p(c["widx"]), ob.p(c["gran"]), ob.p(flat), ob.p(pcm), cap,
                          ob.p(emit), ctypes.byref(bad))
    return rc, emit, pcm


def two_term_overlap(bs0, bs1, channels, t):
    """The device's overlap (vsyn_staged.h, vsyn_overlap_kernel) re-driven in numpy with the oracle's windows: emitted sample s of
    packet i = fl(fl(prev[n_prev/2 + s] * w_prev[..]) + fl(cur[j] * w_cur[j])), each term where its block covers the sample.
    -> (pcm [channels][cap], emit_len)"""
    flags, widx, sizes, blocks, gran, cap = t["flags"], t["widx"], t["sizes"], t["blocks"], t["gran"], t["cap"]
    npk = len(flags)
    pos = 0
    got = np.zeros((channels, cap), np.float32)
    emit_g = np.zeros(npk, np.uint32)
    for i in range(1, npk):
        npv, ncr = int(sizes[i - 1]), int(sizes[i])
        L = npv // 4 + ncr // 4
        wp = np.zeros(npv, np.float32)
        wc = np.zeros(ncr, np.float32)
        ob.oracle().orc_window(bs0, bs1, int(flags[i - 1]), int(widx[i - 1]) & 1, int(widx[i - 1]) >> 1, ob.p(wp))
        ob.oracle().orc_window(bs0, bs1, int(flags[i]), int(widx[i]) & 1, int(widx[i]) >> 1, ob.p(wc))
        s = np.arange(L)
        ip = npv // 2 + s
        jc = ncr // 2 - L + s
        chunk = np.zeros((channels, L), np.float32)
        okp = ip < npv
        chunk[:, okp] = blocks[i - 1][:, ip[okp]] * wp[ip[okp]]
        okc = jc >= 0
        chunk[:, okc] = (chunk[:, okc] + blocks[i][:, jc[okc]] * wc[jc[okc]]).astype(np.float32)
        if gran[i] >= 0:
            L = int(gran[i]) - pos
        got[:, pos:pos + L] = chunk[:, :L]
        emit_g[i] = L
        pos += L
    return got, emit_g


def canonical_zero(a):
    """-0.0 -> +0.0: the overlap test compares numerically, as the reference's PCM and the re-drive may differ in the zero's sign"""
    return (np.asarray(a, np.float32) + np.float32(0.0)).astype(np.float32)


# ---- the tests ----

@pytest.mark.parametrize("n", SIZES)
def test_mdct_tables_and_backward_bit_exact(n):
    orc = ob.oracle()
    m = orc.orc_mdct_new(n)
    ot = np.ctypeslib.as_array(orc.orc_mdct_trig(m), shape=(n + n // 4,))
    orv = np.ctypeslib.as_array(orc.orc_mdct_bitrev(m), shape=(n // 4,))
    assert_ref("mdct_trig_%d" % n, bits(ot))
    assert_ref("mdct_bitrev_%d" % n, orv.astype(np.int32))
    orc.orc_mdct_free(m)
    got = ob.imdct(n, mdct_input(n))
    assert_ref("mdct_backward_%d" % n, bits(got))


@pytest.mark.parametrize("n", CLOSED_FORM_SIZES)
def test_closed_form_agrees_with_reference(n):
    x = closed_form_input(n)
    want = ref_vector("closed_form_%d" % n)
    cf = np.empty(n, np.float64)
    ob.oracle().orc_imdct_closed_form(n, ob.p(x), ob.p(cf))
    assert np.abs(cf - want).max() < 2e-6
    # symmetries stated in SURVEY 8a-7
    assert np.array_equal(want[: n // 2][::-1], -want[: n // 2])
    assert np.array_equal(want[n // 2:][::-1], want[n // 2:])


@pytest.mark.parametrize("bs0,bs1", WINDOW_PAIRS)
def test_windows_bit_exact(bs0, bs1):
    for flag, prev, nxt in WINDOW_CASES:
        n = bs1 if flag else bs0
        b = np.zeros(n, np.float32)
        ob.oracle().orc_window(bs0, bs1, flag, prev, nxt, ob.p(b))
        assert_ref("window_%d_%d_%d%d%d" % (bs0, bs1, flag, prev, nxt), bits(b))


def test_inverse_db_table_bit_exact():
    b = np.ctypeslib.as_array(ob.oracle().orc_inverse_db_table(), shape=(256,))
    assert_ref("inverse_db_table", bits(b))


def test_render_helpers():
    orc = ob.oracle()
    points, lines, sets = render_inputs()
    assert_ref("render_point", np.array([orc.orc_render_point(*(int(v) for v in pt)) for pt in points], np.uint32))
    rendered = []
    for x0, y0, x1, y1, ln in lines:
        a = np.full(ln, 7777, np.uint32)
        orc.orc_render_line(x0, y0, x1, y1, ob.p(a), ln)
        # DDA == closed form per x (the identity the HIP kernel relies on)
        for x in range(x0, min(x1, ln)):
            assert a[x] == orc.orc_render_point(x0, y0, x1, y1, x)
        rendered.append(a)
    assert_ref("render_line", np.concatenate(rendered))
    nb = [(orc.orc_low_neighbor(ob.p(v), idx), orc.orc_high_neighbor(ob.p(v), idx)) for v in sets for idx in range(1, len(v))]
    assert_ref("neighbors", np.array(nb, np.int32))


def floor1_tail(key, cases, accepted=False):
    """orc_floor1_synth on (xs, mult, ys, n) cases against the reference's verdicts (key + "_failed") and curves (key: the inverse-dB
    values of the accepted ones, all n of a block). accepted: every case is one that both decode."""
    orc = ob.oracle()
    want_rc = ref_vector(key + "_failed")
    assert len(want_rc) == len(cases), key
    decoded = []
    for trial, (xs, mult, ys, n) in enumerate(cases):
        got = np.zeros(n, np.float32)
        ro = orc.orc_floor1_synth(ob.p(xs), len(xs), mult, ob.p(ys), n, ob.p(got), None, None, None)
        assert bool(want_rc[trial]) == (ro != 0), (key, trial, ro)
        assert not (accepted and ro), (key, trial, ro)
        if ro == 0:
            decoded.append(bits(got))
    assert_ref(key, np.concatenate(decoded) if decoded else np.zeros(0, np.uint32))


def geometry_floor1_inputs(geom, bs0, bs1):
    """-> (key, [(xs, mult, ys, n)]) of a geometry of floor_geometry_cases.py: X lists whose x[1] is not half the block size"""
    return "floorgeo_%s_%d_%d" % (geom, bs0, bs1), [(c["xs"], c["mult"], c["ys"], c["n"]) for c in fg.floor_cases(geom, bs0, bs1)]


@pytest.mark.parametrize("mult", FLOOR_MULTS)
@pytest.mark.parametrize("posts,n", FLOOR_SHAPES)
def test_floor1_tail_vs_reference(mult, posts, n):
    floor1_tail("floor1_%d_%d_%d" % (mult, posts, n), [(xs, mult, ys, n) for xs, ys in floor1_inputs(mult, posts, n)])


@pytest.mark.parametrize("bs0,bs1", fg.PAIRS)
@pytest.mark.parametrize("geom", fg.GEOMETRIES)
def test_floor1_tail_vs_reference_on_floor_geometries(geom, bs0, bs1):
    """The same on X lists with x[1] above and below half the block size and on floors that both block sizes use (random_xs above
    only draws x[1] == n / 2): the reference decodes every case, the oracle gives its curve over the whole floor vector."""
    key, cases = geometry_floor1_inputs(geom, bs0, bs1)
    assert not ref_vector(key + "_failed").any(), key
    floor1_tail(key, cases, accepted=True)


@pytest.mark.parametrize("bs0,bs1,channels", OVERLAP_CONFIGS)
def test_overlap_add_state_vs_reference(bs0, bs1, channels):
    """oracle decode state == reference VorbisStreamDecodeState on random mixed block sequences (incl. the
    sliding-buffer moves) with a clipping granule on the last packet."""
    for trial, t in enumerate(overlap_inputs(bs0, bs1, channels)):
        key = "overlap_%d_%d_%d_%d" % (bs0, bs1, channels, trial)
        # oracle side: run only the state part by feeding identity "IMDCT": instead use the oracle's own
        # functions through a python re-drive of orc_window + the two-term overlap formula
        got, emit_g = two_term_overlap(bs0, bs1, channels, t)
        assert_ref(key + "_emit", emit_g)
        assert_ref(key + "_pcm", bits(canonical_zero(got)))  # numerically equal (-0.0 == 0.0); the stored PCM is finite
        # and the oracle's own decode state (what orc_submit runs) on the same blocks
        rc, emit_o, pcm_o = overlap_ref_call(ob.oracle(), "orc_overlap_add", bs0, bs1, channels, t)
        assert rc == 0
        assert_ref(key + "_emit", emit_o)
        assert_ref(key + "_pcm", bits(canonical_zero(pcm_o)))


@pytest.mark.parametrize("bs0,bs1,channels", WINFLAG_CONFIGS)
def test_overlap_state_on_disagreeing_window_flags(bs0, bs1, channels):
    """Window flags that disagree with the block sequence (winflag_seq: classes A-D, random flags on short blocks), >= 200 packets.
    The oracle's decode state == the reference's bit for bit, class A included. The device's two-term overlap == the reference bit
    for bit wherever class A is absent; on class A it is off by more than 0.1 — why the device refuses that input
    (VSYN_ST_WINDOW_FLAGS) rather than return different PCM."""
    for trial, t in enumerate(winflag_inputs(bs0, bs1, channels)):
        key = "winflags_%d_%d_%d_%d" % (bs0, bs1, channels, trial)
        a = has_class_a(t["flags"], t["widx"], bs0, bs1)
        assert a == (t["kind"] in ("a", "random") and bs0 < bs1), (key, t["kind"])
        rc, emit_o, pcm_o = overlap_ref_call(ob.oracle(), "orc_overlap_add", bs0, bs1, channels, t)
        assert rc == 0, key
        assert_ref(key + "_emit", emit_o)
        assert_ref(key + "_pcm", bits(canonical_zero(pcm_o)))
        got, emit_g = two_term_overlap(bs0, bs1, channels, t)
        assert np.array_equal(emit_g, emit_o), key
        if not a:
            assert_ref(key + "_pcm", bits(canonical_zero(got)))
        else:
            assert float(np.abs(got - pcm_o).max()) > 0.1, key


@pytest.mark.parametrize("bs0,bs1", [(256, 2048), (1024, 1024)])
def test_oracle_submit_refuses_class_a(bs0, bs1):
    """orc_submit raises VSYN_ST_WINDOW_FLAGS on the short block behind a long block with next_long set (any non-zero byte), at that
    packet, inside a segment and across submits — and never when the block sizes are equal; B / C / D and flags on short blocks pass."""
    from parseoggvorbis_amd import binding
    from tests.workloads import disagreeing_window_flags, fixture_like_spec, synth_batch
    spec = fixture_like_spec(2, bs0, bs1)
    rng = np.random.default_rng(5)
    blk = np.array([1, 1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 0, 0, 1, 1], np.uint8)
    prev, nxt = disagreeing_window_flags(rng, blk, bs0, bs1)
    b = synth_batch(spec, 1, len(blk), blk, seed=3, prev_long=prev, next_long=nxt)
    assert ob.OracleSynth(spec, 1).submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"])["rc"] == 0
    for byte in (1, 2, 0x80, 255):
        pk = b["packets"].copy()
        pk["next_long"][9] = byte  # long 9, short 10
        w = ob.OracleSynth(spec, 1).submit_host(pk, b["segments"], b["ys"], b["residue"], b["plane_stride"])
        if bs0 < bs1:
            assert (w["rc"], w["flags"], w["first_bad"]) == (binding.VSYN_ERR_STREAM, binding.VSYN_ST_WINDOW_FLAGS, 10)
        else:
            assert w["rc"] == 0
    # across submits: the first ends on long block 9, the second starts with short block 10
    pk = b["packets"].copy()
    pk["next_long"][9] = 1
    n_of = np.where(blk == 1, bs1, bs0)
    off = np.concatenate([[0], np.cumsum(2 * (n_of // 2))])
    orc = ob.OracleSynth(spec, 1)
    rcs = []
    for a, e in ((0, 10), (10, len(blk))):
        seg = b["segments"].copy()
        seg["num_packets"], seg["flags"] = e - a, 1 if a == 0 else 0
        w = orc.submit_host(pk[a:e], seg, b["ys"][a:e], b["residue"][off[a]:off[e]], b["plane_stride"])
        rcs.append((w["rc"], w["flags"], w["first_bad"]))
    assert rcs[0][0] == 0
    assert rcs[1] == ((binding.VSYN_ERR_STREAM, binding.VSYN_ST_WINDOW_FLAGS, 0) if bs0 < bs1 else (0, 0, 0xFFFFFFFF))
