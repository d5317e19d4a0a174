"""Setups with several modes per block size, a floor per channel and table numbers up to 63 (multimode_cases.py), on the CPU: the
case table keeps the promises its GPU module relies on (they are conditions on the batches, checked here and not on the device),
the oracle's integer taps equal the plain integer model of floor_geometry_cases.py with every row on the floor of its own channel,
and the oracle's PCM stays inside the per-packet gate of synth_model.py (G = 96, unchanged)."""
import numpy as np
import pytest

from oracle import oracle_binding as ob
from tests import floor_geometry_cases as fg
from tests import multimode_cases as mm
from tests import synth_model as sm

KEYS = sorted(mm.CASES, key=mm.case_id)
WORST = {}


def _segments(b):
    return [(int(sg["first_packet"]), int(sg["num_packets"])) for sg in b["segments"]]


def _long(spec, b):
    return np.array([spec.modes[int(m)][0] for m in b["packets"]["mode"]], bool)


def test_setups_are_what_the_table_says():
    for key in KEYS:
        case, bs0, bs1, channels, variant = key
        spec, longs, shorts = mm.make_setup(key)
        assert (spec.channels, spec.blocksize0, spec.blocksize1) == (channels, bs0, bs1)
        used = longs + shorts
        used_floors = sorted({f for k in used for f in spec.mappings[spec.modes[k][1]][1]})
        posts = [len(spec.floors[f][1]) for f in (range(len(spec.floors)) if case != "numbering" else used_floors)]
        assert len(set(posts)) == len(posts), (key, posts)  # no two floors share a post count
        for f, (mult, xs) in enumerate(spec.floors):
            halves = {(spec.blocksize1 if bf else spec.blocksize0) // 2 for bf, mp in spec.modes if f in spec.mappings[mp][1]}
            assert len(halves) == 1 and xs[:2] == [0, halves.pop()] and len(set(xs)) == len(xs) and max(xs) == xs[1], (key, f)
            assert len(xs) <= (64 if mm.CASES[key] == mm.TUNED else 65), (key, f)
            assert len(xs) < 4 or xs[2:] != sorted(xs[2:]), (key, f)  # header order is not the sorted order
        assert all(spec.modes[k][0] for k in longs) and not any(spec.modes[k][0] for k in shorts), key
        thresholds = {len(spec.floors[f][1]) for f in used_floors}
        if case in ("long_modes", "long_modes_u"):
            assert thresholds == {2, 9, 12, 32 if variant == 64 else 33, variant}, key
            for k in used:  # modes, mappings and floors numbered independently
                mp = spec.modes[k][1]
                assert len({k, mp, spec.mappings[mp][1][0]}) == 3, (key, k)
            assert all(cp == ([(0, 1)] if channels == 2 else []) for cp, _ in spec.mappings)
        if case == "channel_floors":
            assert {2, 9, 12, 32, 33, variant} == thresholds, key
            assert all(len(set(chf)) == 2 for _, chf in spec.mappings), key
            if channels == 3:
                assert all(cp == [(0, 1), (1, 2)] and chf[0] == chf[2] != chf[1] for cp, chf in spec.mappings)
            a, b = (spec.mappings[spec.modes[k][1]][1][:2] for k in longs[:2])
            assert a == b[::-1] and sorted(len(spec.floors[f][1]) for f in a) == [32, 33], key
        if case == "numbering":
            assert len(spec.modes) == len(spec.mappings) == len(spec.floors) == 64
            assert spec.modes[0][0] == 1 and spec.modes[63] == (0, 63) and spec.mappings[63][1] == [63] * channels
            assert tuple(sorted(used)) == mm.NUMBERING_USED
            assert {k & 3 for k in used} == {0, 1, 2, 3}  # every byte of a mode_mapping dword
            for half in (lambda k: k < 32, lambda k: k >= 32):  # both words of the long_modes bitmap, both block sizes in each
                assert {spec.modes[k][0] for k in used if half(k)} == {0, 1}
            assert len({tuple(cp) for cp, _ in spec.mappings}) == 1  # one coupling list throughout
        if case == "couplings_disagree":
            cps = [spec.mappings[spec.modes[k][1]][0] for k in longs]
            assert cps == [[(0, 1)], [(1, 0)] if variant == "swapped" else []], key


@pytest.mark.parametrize("key", KEYS, ids=mm.case_id)
def test_batches_keep_the_promises_of_the_case_table(key):
    spec, bb = mm.batches(key)
    case = key[0]
    C = spec.channels
    for kind, b in bb.items():
        assert len(b["segments"]) <= 3 and all(n <= 48 for _, n in _segments(b))
        lng, posts = _long(spec, b), mm.row_posts(spec, b)
        if kind == "mixed":  # every mode the case names occurs
            assert set(int(m) for m in b["packets"]["mode"]) == set(sum(mm.make_setup(key)[1:], [])), key
        # consecutive packets of one block size whose floors differ in post count, for every channel, at both block sizes
        for c in mm.CLAIMS[key]:
            for size in ((0, 1) if kind == "mixed" and len(mm.make_setup(key)[2]) > 1 else (1,)):
                hit = [q for a, n in _segments(b) for q in range(a + 1, a + n)
                       if lng[q] == lng[q - 1] == bool(size) and posts[q, c] != posts[q - 1, c]]
                assert hit, (key, kind, c, size)
        if kind == "mixed" and len(mm.make_setup(key)[2]) > 1:
            mp = np.array([spec.modes[int(m)][1] for m in b["packets"]["mode"]])
            at_transition = 0
            for a, n in _segments(b):
                for q in range(a, a + n - 7):  # every window of eight consecutive short packets holds a mapping change
                    if not lng[q:q + 8].any():
                        assert len(set(mp[q:q + 8])) > 1, (key, q)
                shorts = [q for q in range(a, a + n) if not lng[q]]
                for i, j in zip(shorts[:-1], shorts[1:]):  # the last short packet before a long stretch and the first one behind it
                    at_transition += j - i > 1 and mp[i] != mp[j]
            assert at_transition, key
        if kind == "long":
            assert lng.all()
            for a, n in _segments(b):
                assert n == mm.LONG_PACKETS
            # a floor change on the first packet, the last packet and the halo of a run, for run lengths 3 and 4 (4 is also what
            # fused_pick_run_len plans for a batch this small: "never below 4")
            for R in (3, 4):
                f = l = h = 0
                for a, n in _segments(b):
                    for qa in range(R, n, R):
                        ch = lambda q: a + q < a + n and q >= 1 and posts[a + q, 0] != posts[a + q - 1, 0]
                        f += ch(qa)
                        h += ch(qa - 1)
                        l += ch(qa + R - 1)
                assert f and l and h, (key, R, f, l, h)
            a, n = _segments(b)[2]  # the stream with single changes: on a halo (11) and on a run's first packet (24), nowhere else
            changes = [q for q in range(1, n) if posts[a + q, 0] != posts[a + q - 1, 0]]
            assert changes == [11, 24] and 12 % 3 == 12 % 4 == 24 % 3 == 24 % 4 == 0, (key, changes)
        if case == "channel_floors":
            fl = mm.row_floors(spec, b).ravel()
            pc = posts.ravel()
            for w in range(0, len(fl) - 63, 64):
                assert len(set(fl[w:w + 64])) >= 3 and pc[w:w + 64].min() <= 32 < pc[w:w + 64].max(), (key, kind, w)
            used = b["packets"]["floor_used"]
            assert (used != (1 << C) - 1).any() and (used != 0).any()
            if kind == "long" and C == 2:  # adjacent rows on the register form (32 posts) and the LDS form (33) of the unwrap
                assert any(sorted(posts[q]) == [32, 33] for q in range(len(posts)))


@pytest.mark.parametrize("key", KEYS, ids=mm.case_id)
def test_oracle_taps_equal_the_integer_model(key):
    """floor_final and floor_curve of the oracle == the integer model with each row on its own channel's floor, bit for bit; rc 0
    and no status flag; the oracle's emit lengths and PCM inside the per-packet gate of synth_model.py."""
    spec, bb = mm.batches(key)
    for kind, b in bb.items():
        ctx = (mm.case_id(key), kind)
        w = ob.OracleSynth(spec, len(b["segments"])).submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"],
                                                                 want_taps=True)
        assert (w["rc"], w["flags"], w["first_bad"]) == (0, 0, 0xFFFFFFFF), ctx
        final, crv = fg.model_taps(spec, b)
        assert np.array_equal(w["taps"]["floor_final"], final), ctx
        assert np.array_equal(w["taps"]["floor_curve"], crv), ctx
        WORST[ctx] = sm.check_model(w, spec, b, ctx=ctx)  # (asserts the model's frame counts too)


def test_ring_plan_of_the_long_batches():
    """The all-long batches run in ring groups at run lengths 3 and 4, beside per-run groups at 4 (vsyn_fused.h, ring_ok)."""
    for R in (3, 4):
        ring = mm.ring_groups(mm.LONG_STREAMS, mm.LONG_PACKETS, R)
        groups = -(-mm.LONG_STREAMS * (-(-mm.LONG_PACKETS // R)) * 2 // 16)
        assert 0 < len(ring) <= groups and (R == 3 or len(ring) < groups), (R, ring, groups)


def test_synth_batch_without_modes_is_unchanged():
    """modes=None reproduces the batches from before the keyword, byte for byte: the digests test_synth_model_cpu.py holds."""
    from tests.test_synth_model_cpu import test_synth_batch_defaults_unchanged
    test_synth_batch_defaults_unchanged()


def test_synth_batch_modes_forms_agree():
    """A list and a callable give the same batch, and the first-long / first-short modes given explicitly give the default batch."""
    from tests.test_synth_model_cpu import _digest
    from tests.workloads import fixture_like_spec, synth_batch
    spec = fixture_like_spec(2)
    base = synth_batch(spec, 2, 22, "mixed", seed=4, granule_last=True)
    m = [int(v) for v in base["packets"]["mode"]]
    assert _digest(synth_batch(spec, 2, 22, seed=4, granule_last=True, modes=m)) == _digest(base)
    assert _digest(synth_batch(spec, 2, 22, seed=4, granule_last=True, modes=lambda s, q: m[s * 22 + q])) == _digest(base)


def test_zz_print_the_oracles_worst_ratio_per_case():
    print("\noracle worst max|d| / (2^-24 s) per case (gate %g):" % sm.G)
    for k in sorted(WORST):
        print("  %-40s %-6s %5.1f" % (k + (WORST[k],)))
    assert WORST and all(v <= sm.G for v in WORST.values())
