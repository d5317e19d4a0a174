"""Setups with several modes per block size, a floor per channel and table numbers up to 63 (multimode_cases.py) on every synthesis
path of the device. The kernels cache what every other test holds constant: the lane constants of the current floor and the
prefetched coded row (vsyn_fused.h), the mapping of a packed pass (both fused kernels), the floors of a wave of rows
(floor1_unwrap_rows) and the modes of a wave of packets (vsyn_prep.h). A stale cache gives wrong PCM with flags == 0.

Per case (mixed and all-long batch, 2-3 streams of at most 48 packets):
  - floor_final and floor_curve of the fused kernel's tap variant behind the preparation kernel, behind the chained pre-kernels and
    behind the hidden pre-kernels, and of the staged kernels == the integer model == the oracle, bit for bit; after_envelope of the
    staged kernels == the oracle's, bit for bit; emit_len exact; PCM inside test_gpu_parity's gates (TOL and the per-packet model gate);
  - PCM of the plain fused kernel bit-identical to its tap variant;
  - the kernel that ran, read from the kernel profile, and vsyn_fused_paths equal the case table's.
Ring mode (long_modes, all-long, VSYN_RUN_LEN 3 / 4 / planned), streams cut across submits where the floor changes, the same stream
at either end of a batch of other modes, and synth_18 / synth_19 (make_synth_ogg.py --floors per_mode) from Ogg bytes.
Measured on one MI355X: 4.2 s for the module's 32 tests (the slowest case 0.7 s); the device's worst model ratio 17.1 (gate 96).

Which case is built to catch which stale cache (by the conditions test_multimode_cpu.py asserts on the batches):
  the `cur_floor != f` reload of vsyn_fused.h             long_modes-256-2048: consecutive long packets on floors of 12 / 32 / 64 posts
                                                           (every path, ring mode: on a run's first packet, last packet and halo)
  the `pin.mapping == pi.mapping` term of vrow_ok          the same packets, together with the reload: the prefetched row is only used
                                                           where cur_floor == f, and then it was fetched with that floor's sorted index,
                                                           so the term alone is implied by the reload check (no output depends on it)
  "same mapping" of a packed pass                          long_modes-256-2048 mixed (fused_short_pass: a mapping change in every
                                                           window of eight short packets), long_modes_u-* (both block sizes)
  the `mine` mask of floor1_unwrap_rows                    channel_floors-*: adjacent rows on floors of 32 and 33 posts, three floors
                                                           in every 64 rows
  the 1ull of long_modes                                   numbering-*: long modes 32 and 62 (bits of the bitmap's upper word)"""
import os

import numpy as np
import pytest

from oracle import oracle_binding as ob
from parseoggvorbis_amd import binding
from tests import floor_geometry_cases as fg
from tests import multimode_cases as mm
from tests import synth_model as sm
from tests.test_gpu_parity import HIDDEN_PRE, TOL, bits, check
from tests.workloads import concat_batches, packet_blocks, synth_batch

pytestmark = pytest.mark.gpu
PRE = binding.VSYN_SUBMIT_PRE_KERNELS
STAGED = binding.VSYN_SUBMIT_STAGED
STAGED_KERNEL = "vsyn_imdct_staged_kernel"
KEYS = sorted(mm.CASES, key=mm.case_id)
RAN = {}    # case id -> kernels that ran
WORST = {}  # case id -> the device's worst model ratio
_WANT = {}


def oracle(key, kind):
    """The oracle's result (taps included) and the integer model's taps of a case's batch, computed once"""
    if (key, kind) not in _WANT:
        spec, bb = mm.batches(key)
        b = bb[kind]
        w = ob.OracleSynth(spec, len(b["segments"])).submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"],
                                                                 want_taps=True)
        assert (w["rc"], w["flags"]) == (0, 0), (key, kind)
        final, crv = fg.model_taps(spec, b)
        assert np.array_equal(w["taps"]["floor_final"], final) and np.array_equal(w["taps"]["floor_curve"], crv), (key, kind)
        _WANT[(key, kind)] = (w, final, crv)
    return _WANT[(key, kind)]


def _submit(g, b, **kw):
    g.reset()
    got = g.submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"], **kw)
    _, launches, kernel = g.profile_read()
    assert launches, kernel
    return got, kernel


def _taps_equal(got, final, crv, ctx):
    bad = np.flatnonzero(got["taps"]["floor_final"] != final)
    assert not len(bad), (ctx, "floor_final", len(bad), bad[:4], got["taps"]["floor_final"][bad[:4]], final[bad[:4]])
    bad = np.flatnonzero(got["taps"]["floor_curve"] != crv)
    assert not len(bad), (ctx, "floor_curve", len(bad), bad[:4], got["taps"]["floor_curve"][bad[:4]], crv[bad[:4]])


@pytest.mark.parametrize("key", KEYS, ids=mm.case_id)
def test_case_on_every_path(key):
    spec, bb = mm.batches(key)
    paths, plain_kernel, tap_kernel = mm.CASES[key]
    g = binding.Synth(spec, max_streams=4)
    g.profile(1)
    assert g.fused_paths & 3 == paths, (mm.case_id(key), g.fused_paths)
    for kind, b in bb.items():
        ctx = (mm.case_id(key), kind)
        want, final, crv = oracle(key, kind)
        # the fused kernel's tap variant, behind vsyn_prep_kernel
        tap, kernel = _submit(g, b, want_taps="features")
        assert kernel == tap_kernel, (ctx, kernel)
        assert tap["flags"] == 0, (ctx, tap["flags"], tap["first_bad"])
        _taps_equal(tap, final, crv, ctx + (kernel,))
        check(tap, want, model=(spec, b))
        WORST[ctx] = sm.check_model(tap, spec, b, ctx=ctx)
        # the plain fused kernel: the tap changes nothing else
        plain, kernel = _submit(g, b)
        assert kernel == plain_kernel, (ctx, kernel)
        assert plain["flags"] == 0, ctx
        assert np.array_equal(plain["emit_len"], tap["emit_len"]) and np.array_equal(bits(plain["pcm"]), bits(tap["pcm"])), ctx
        # the chained pre-kernels in front of the same kernel, on the caller's stream and hidden on the internal one
        for flags, name in ((PRE, "pre-kernels"), (HIDDEN_PRE, "hidden pre-kernels")):
            pre, kernel = _submit(g, b, want_taps="features", flags=flags)
            assert kernel == tap_kernel, (ctx, name, kernel)
            assert pre["flags"] == 0, (ctx, name)
            _taps_equal(pre, final, crv, ctx + (name, kernel))
            assert np.array_equal(pre["emit_len"], want["emit_len"]), (ctx, name)
            assert np.array_equal(bits(pre["pcm"]), bits(tap["pcm"])), (ctx, name)
        # the staged kernels (integer curve), with the envelope tap
        staged, kernel = _submit(g, b, want_taps=True, flags=STAGED)
        assert kernel == STAGED_KERNEL, (ctx, kernel)
        assert staged["flags"] == 0, ctx
        _taps_equal(staged, final, crv, ctx + (kernel,))
        assert np.array_equal(bits(staged["taps"]["after_envelope"]), bits(want["taps"]["after_envelope"])), ctx
        check(staged, want, model=(spec, b))
        RAN.setdefault(mm.case_id(key), set()).update((tap_kernel, plain_kernel, STAGED_KERNEL))


LONG_MODES = ("long_modes", 256, 2048, 2, 64)
CHANNEL_FLOORS = ("channel_floors", 256, 2048, 2, 64)


def _with_run_len(monkeypatch, run_len, spec, max_streams):
    if run_len:
        monkeypatch.setenv("VSYN_RUN_LEN", str(run_len))
    else:
        monkeypatch.delenv("VSYN_RUN_LEN", raising=False)
    g = binding.Synth(spec, max_streams=max_streams)
    monkeypatch.delenv("VSYN_RUN_LEN", raising=False)
    return g


def test_ring_mode_same_bits_for_every_run_length(monkeypatch):
    """long_modes' all-long batch with run lengths 3, 4 and the planned one (4 for a batch this small): ring groups at both lengths
    and per-run groups beside them at 4 (mm.ring_groups restates ring_ok; test_multimode_cpu.py asserts the plan and that a floor
    change falls on a run's first packet, last packet and halo). The same bits whatever the run length; oracle and model gates."""
    spec, bb = mm.batches(LONG_MODES)
    b = bb["long"]
    want, final, crv = oracle(LONG_MODES, "long")
    for R in (3, 4):
        ring = mm.ring_groups(len(b["segments"]), mm.LONG_PACKETS, R)
        assert ring and (R == 3 or len(ring) < -(-len(b["segments"]) * -(-mm.LONG_PACKETS // R) * 2 // 16)), (R, ring)
    ref = None
    for rl in (3, 4, 0):
        g = _with_run_len(monkeypatch, rl, spec, len(b["segments"]))
        g.profile(1)
        got, kernel = _submit(g, b, want_taps="features")
        assert kernel == "vsyn_fused_tap_kernel" and got["flags"] == 0, (rl, kernel)
        _taps_equal(got, final, crv, ("ring", rl))
        check(got, want, model=(spec, b))
        plain, kernel = _submit(g, b)
        assert kernel == "vsyn_fused_kernel", (rl, kernel)
        assert np.array_equal(bits(plain["pcm"]), bits(got["pcm"])), rl
        if ref is None:
            ref = got
        else:
            assert np.array_equal(bits(got["pcm"]), bits(ref["pcm"])), rl


def _floor_change(spec, b, s, lng_only=False):
    """A packet of segment s (not among its first three or last two) whose floor differs in post count from its predecessor's"""
    posts = mm.row_posts(spec, b)
    a, n = int(b["segments"][s]["first_packet"]), int(b["segments"][s]["num_packets"])
    for q in range(a + 3, a + n - 2):
        if (posts[q] != posts[q - 1]).any() and (not lng_only or (spec.modes[int(b["packets"]["mode"][q])][0]
                                                                  and spec.modes[int(b["packets"]["mode"][q - 1])][0])):
            return q - a
    raise AssertionError("no floor change")


@pytest.mark.parametrize("flags", [0, PRE, STAGED])
@pytest.mark.parametrize("key,kind,stream", [(LONG_MODES, "long", 2), (LONG_MODES, "mixed", 1), (CHANNEL_FLOORS, "long", 0),
                                             (CHANNEL_FLOORS, "mixed", 0)])
def test_streaming_cut_where_the_floor_changes(key, kind, stream, flags):
    """A stream cut into submits at a packet whose floor differs from its predecessor's, and one packet to either side: emit_len as
    in the single submit; PCM bit-identical on the staged path, within TOL on the fused path (test_streaming_across_submits)."""
    spec, bb = mm.batches(key)
    b = bb[kind]
    a, npk = int(b["segments"][stream]["first_packet"]), int(b["segments"][stream]["num_packets"])
    n_of, off = packet_blocks(spec, b["packets"], b["segments"])
    end = np.append(off, off[-1] + spec.channels * n_of[-1] // 2)
    seg1 = b["segments"][stream:stream + 1].copy()
    seg1["stream"], seg1["first_packet"], seg1["residue_off"] = 1, 0, 0
    one = binding.Synth(spec, max_streams=2).submit_host(b["packets"][a:a + npk], seg1, b["ys"][a:a + npk], b["residue"][end[a]:end[a + npk]],
                                                        b["plane_stride"], flags=flags)
    assert (one["rc"], one["flags"]) == (0, 0)
    total = int(one["emit_len"].sum())
    t = _floor_change(spec, b, stream)
    g = binding.Synth(spec, max_streams=2)
    parts = []
    cuts = [0, t - 1, t, t + 1, npk]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        seg = seg1.copy()
        seg["num_packets"], seg["flags"] = hi - lo, 1 if lo == 0 else 0
        r = g.submit_host(b["packets"][a + lo:a + hi], seg, b["ys"][a + lo:a + hi], b["residue"][end[a + lo]:end[a + hi]], b["plane_stride"],
                          flags=flags)
        assert (r["rc"], r["flags"]) == (0, 0), (lo, hi)
        assert np.array_equal(r["emit_len"], one["emit_len"][lo:hi]), (lo, hi)
        parts.append(r["pcm"][0][:, :int(r["emit_len"].sum())])
    got = np.concatenate(parts, axis=1)
    if flags == STAGED:
        assert np.array_equal(bits(got), bits(one["pcm"][0][:, :total]))
    else:
        assert np.abs(got - one["pcm"][0][:, :total]).max() < TOL * max(1.0, float(np.abs(one["pcm"]).max()))


@pytest.mark.parametrize("key", [LONG_MODES, ("long_modes_u", 128, 1024, 2, 65), CHANNEL_FLOORS], ids=mm.case_id)
def test_position_independence(key):
    """The same stream as segment 0 and as the last segment of a batch whose other segments use other modes: the same bits."""
    spec, bb = mm.batches(key)
    _, longs, shorts = mm.make_setup(key)
    npk = 33
    mine = synth_batch(spec, 1, npk, seed=41, modes=mm.mixed_pattern(longs, shorts, 1, npk)[0])
    others = [synth_batch(spec, 1, npk, seed=42, modes=[longs[-1]] * npk),
              synth_batch(spec, 1, npk, seed=43, modes=mm.mixed_pattern(longs[::-1], shorts[::-1], 2, npk)[1]),
              synth_batch(spec, 1, 7, seed=44, modes=[shorts[-1]] * 7)]
    first = concat_batches([mine] + others)
    last = concat_batches(others + [mine])
    want = ob.OracleSynth(spec, 4).submit_host(first["packets"], first["segments"], first["ys"], first["residue"], first["plane_stride"])
    g = binding.Synth(spec, max_streams=4)
    a = g.submit_host(first["packets"], first["segments"], first["ys"], first["residue"], first["plane_stride"])
    check(a, want, model=(spec, first))
    g.reset()
    z = g.submit_host(last["packets"], last["segments"], last["ys"], last["residue"], last["plane_stride"])
    assert (a["flags"], z["flags"]) == (0, 0)
    assert np.array_equal(a["emit_len"][:npk], z["emit_len"][-npk:])
    assert np.array_equal(bits(a["pcm"][0]), bits(z["pcm"][3]))
    for k in range(3):
        assert np.array_equal(bits(a["pcm"][k + 1]), bits(z["pcm"][k])), k


def test_per_mode_floor_streams_end_to_end():
    """synth_18 (stereo 256/2048) and synth_19 (three channels, 128/1024), a floor per (mapping, submap) and several modes per block
    size, from Ogg bytes through the corpus decoder: frame counts equal the reference's, PCM within 4e-6 of max(1, peak) as for the
    other synthetic streams."""
    from tests.test_gpu_host_decoder import GOLDEN, _run_corpus
    names = ["synth_18", "synth_19"]
    gold = [np.load(os.path.join(GOLDEN, n + ".npz")) for n in names]
    for z in gold:
        bf = z["mode_blockflag"]
        assert (bf == 0).sum() >= 2 and (bf == 1).sum() >= 2 and int(z["num_floors"]) > 2
        assert any(len(set(int(f) for f in z["chfloor_m%d" % k])) > 1 for k in range(int(z["mode_mapping"].max()) + 1))
    blobs = [open(os.path.join(GOLDEN, n + ".ogg"), "rb").read() for n in names]
    frames, sums, ok, pcm, stats = _run_corpus(blobs, [int(z["channels"]) for z in gold], threads=2, feeders=1, files_per_submit=2, cap=32768)
    for i, z in enumerate(gold):
        want = z["pcm"]
        assert ok[i] and frames[i] == want.shape[1], (names[i], frames[i], want.shape)
        err = float(np.abs(pcm[i][:, :frames[i]] - want).max())
        assert err <= 4e-6 * max(float(np.abs(want).max()), 1.0), (names[i], err)


def test_zz_every_case_ran_on_the_kernel_named():
    print("\nkernels and the device's worst max|d| / (2^-24 s) per case (gate %g):" % sm.G)
    for key in KEYS:
        cid = mm.case_id(key)
        print("  %-40s %-52s %s" % (cid, ", ".join(sorted(RAN.get(cid, ()))),
                                    "  ".join("%s %.1f" % (k, WORST[(cid, k)]) for k in ("mixed", "long") if (cid, k) in WORST)))
    assert all(RAN[mm.case_id(key)] == {mm.CASES[key][1], mm.CASES[key][2], STAGED_KERNEL} for key in KEYS if mm.case_id(key) in RAN)
