"""GPU: the residue VQ kernel (csrc/vsyn_vq.h) past stereo 2048 and past one packet per wave. tests/test_gpu_vq.py pins the stage
on the fixtures' shapes; here are the shapes and the states it does not reach: 3 to 15 channels per submap in every format, every
block size, a wave that decodes packet after packet (its cached per-residue records, its channel list, its staged entry numbers and
what a longer packet left behind), entry counts at the edge of the LDS staging buffer, per-pass counts at the edge of the scan's
16-bit halves, the device entry point, and a status raised on a wave's later visit.

The contract is the suite's: residue bit for bit against the oracle (oracle/, pinned to the reference where the reference is a
valid judge, and to tests/vq_model.py on every setup used here: tests/test_vq_model_cpu.py). One case per group also compares with
vq_model directly and gates the PCM against the float64 synthesis model (tests/synth_model.py).

Every submit is preceded by a float submit of the same size whose residue is a constant, so that the residue buffer of the handle
holds non-zero values wherever the kernel fails to store or to zero-fill.

VSYN_VQ_GRID (tools/README.md) caps the kernel's grid so that a small batch makes every wave walk several packets; the launch shape
is read from the VSYN_DEBUG line of vsyn_attach_vq and asserted."""
import re

import numpy as np
import pytest

from oracle import oracle_binding as ob
from parseoggvorbis_amd.binding import VSYN_ERR_STREAM, VSYN_ST_BAD_MODE, VSYN_ST_BAD_VQ, Synth, VsynError
from tests import synth_model, vq_cases, vq_model
from tests.workloads import (assemble_vq_batch, fixture_like_spec, random_own_mask, synthetic_vq_spec, vq_pool_packet,
                             vq_submap_shapes)

pytestmark = pytest.mark.gpu
LAUNCH = re.compile(r"\[vsyn\] vq launch: (\d+) workgroups, (\d+) waves per workgroup, (\d+) B LDS, tables in (LDS|global memory)")
DIRT = 3.0


def _attach(syn, vqs, capfd):
    """attach_vq (the setup must be accepted) -> (workgroups, waves per workgroup, LDS bytes, tables in LDS) of the launch line."""
    capfd.readouterr()
    syn.attach_vq(vqs)
    m = LAUNCH.findall(capfd.readouterr().err)
    assert m, "no VQ launch line: VSYN_DEBUG must be set before the handle is created"
    g, w, lds, home = m[-1]
    assert bool(syn.fused_paths & 0x100) == (home == "LDS")
    return int(g), int(w), int(lds), home == "LDS"


def _expected(spec, vqs, pkts, model=False):
    """The oracle's residue of every packet of the list (one call per distinct packet) -> list of arrays."""
    cache = {}
    for k in pkts:
        if id(k) not in cache:
            rc, res = ob.residue_vq(vqs, k["mapping"], spec.channels, k["n2"], k["used"], k["cls"], k["ent"])
            assert rc == 0
            if model:
                m = vq_model.residue_vq(vqs, k["mapping"], spec.channels, k["n2"], k["used"], k["cls"], k["ent"])
                assert np.array_equal(m.view(np.uint32), res.view(np.uint32))
            cache[id(k)] = res
    return [cache[id(k)] for k in pkts]


def _ys(syn, P):
    ys = np.zeros((P, syn.channels, syn.ys_stride), np.uint16)
    ys[:, :, :2] = 40  # a flat floor well above the quietest one: the PCM gate then has something to measure
    return ys


def _submit(syn, b, dirty=True):
    P, total = len(b["packets"]), int(b["res_off"][-1])
    ys = _ys(syn, P)
    if dirty:
        clean = b["packets"].copy()
        clean["mode"][clean["mode"] >= len(syn.spec.modes)] = 0  # (a bad mode takes a short block's room: so does mode 0)
        syn.submit_host(clean, b["segments"], ys, np.full(total, DIRT, np.float32), b["plane_stride"])
    out = syn.submit_host_vq(b["packets"], b["segments"], ys, b["vq_packets"], b["cls"], b["entries"], total, b["plane_stride"])
    out["ys"] = ys
    return out


def _assert_bits(out, b, want, skip=()):
    """Residue bit for bit, packet by packet (the first packet that differs is named)."""
    got = out["residue"]
    for p, w in enumerate(want):
        if p in skip:
            continue
        g = got[int(b["res_off"][p]):int(b["res_off"][p]) + w.size]
        if not np.array_equal(g.view(np.uint32), w.view(np.uint32)):
            bad = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
            raise AssertionError("packet %d: %d of %d values differ, first at %d: got %r want %r" % (p, bad.size, w.size, bad[0], g[bad[0]],
                                                                                                  w[bad[0]]))


def _check_pcm(out, spec, b):
    assert synth_model.agreeing_flags(spec, b["packets"], b["segments"])
    synth_model.check_model(out, spec, dict(packets=b["packets"], segments=b["segments"], ys=out["ys"], residue=out["residue"],
                                            plane_stride=b["plane_stride"]))


def _random_packets(spec, vqs, streams, per, pattern, seed, forced_own=()):
    """streams * per random packets, block flags from `pattern` (mode = first mode of that block flag), about 30 % with a partial
    floor_used; forced_own: masks given to the first packets instead."""
    rng = np.random.default_rng(seed)
    mode_of = {int(bf): [i for i, (f, _) in enumerate(spec.modes) if int(f) == int(bf)][0] for bf in (0, 1)}
    pkts = []
    for p in range(streams * per):
        own = forced_own[p] if p < len(forced_own) else random_own_mask(rng, spec.channels)
        pkts.append(vq_pool_packet(spec, vqs, mode_of[pattern[(p % per) % len(pattern)]], own, rng))
    return pkts


# ---- a. channels x formats ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(vq_cases.CHANNEL_CASES))
def test_channels_and_formats(name, capfd, monkeypatch):
    """3, 5 and 6 channels in one format 2 vector (per-element de-interleave with e % nch, zero-fill runs that depend on the channel,
    begin and the last partition's end no multiples of the channel count), 3 and 6 channels side by side in formats 1 and 0 (pj / vch,
    the [vector][partition] classification layout, the per-vector used mask behind chained couplings, more channels than sub_chan4
    holds), the 5.1 split over two submaps, and begins that take both unaligned store fallbacks; long and short blocks mixed,
    5 streams x 12 packets at 128/1024."""
    monkeypatch.setenv("VSYN_DEBUG", "1")
    spec, vqs = vq_cases.channel_case(name)
    forced = [0b100, 0b100, 0b001, 0b010] if name == "chain3" else []
    pkts = _random_packets(spec, vqs, 5, 12, [1, 0, 1, 1, 0, 0, 1], seed=len(name) + spec.channels, forced_own=forced)
    partial = sum(k["own"] != (1 << spec.channels) - 1 for k in pkts)
    assert partial >= 8 and any(k["long"] for k in pkts[:4]) and any(not k["long"] for k in pkts[:4])
    syn = Synth(spec, max_streams=5)
    _attach(syn, vqs, capfd)  # accepted
    b = assemble_vq_batch(spec, pkts, 5)
    want = _expected(spec, vqs, pkts, model=name in ("f2x5", "chain3"))
    out = _submit(syn, b)
    assert out["rc"] == 0, out
    _assert_bits(out, b, want)
    assert max(float(np.abs(w).max()) for w in want) > 0
    if name in ("f2x5", "chain3"):
        _check_pcm(out, spec, b)


# ---- b. block sizes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs0,bs1", vq_cases.BLOCK_PAIRS)
def test_block_sizes(bs0, bs1, capfd, monkeypatch):
    """Stereo at the smallest, the largest and equal block sizes. n2 = 32: a residue that begins behind the vector (no partition:
    the channel is zero fill only) and one with a single partition; 8192: 1024 partitions of 8 = 8192 slots, the stage's limit."""
    monkeypatch.setenv("VSYN_DEBUG", "1")
    spec, vqs = vq_cases.block_case(bs0, bs1)
    per = 4 if bs1 == 8192 else 8
    pkts = _random_packets(spec, vqs, 3, per, [1, 0, 0, 1], seed=bs0 + bs1)
    syn = Synth(spec, max_streams=3)
    _attach(syn, vqs, capfd)  # accepted, 8192 slots included
    b = assemble_vq_batch(spec, pkts, 3)
    want = _expected(spec, vqs, pkts, model=bs0 == 64)
    if bs0 == 64:  # the short blocks: channel 0 has no partition at all, channel 1 exactly one
        assert vq_submap_shapes(vqs, 0, 2, 32) == [(1, 0), (1, 1)]
        short = [w for k, w in zip(pkts, want) if not k["long"] and k["used"] == 3]
        assert short and not any(w[:32].any() for w in short) and any(w[32:].any() for w in short)
    if bs1 == 8192:
        assert vq_submap_shapes(vqs, 1, 2, 4096) == [(1, 1024)]
    out = _submit(syn, b)
    assert out["rc"] == 0, out
    _assert_bits(out, b, want)
    if bs0 == 64:
        _check_pcm(out, spec, b)


def test_one_partition_beyond_the_slot_limit_is_refused():
    spec, vqs = vq_cases.block_case(64, 8192, extra_partition=True)
    syn = Synth(spec, max_streams=1)
    with pytest.raises(VsynError, match="8192"):
        syn.attach_vq(vqs)


# ---- c. the packet walk -------------------------------------------------------------------------------------------------------
def _windows(seq, n):
    return [seq[i:i + n] for i in range(len(seq) - n + 1)]


def _assert_transitions(visits):
    """visits: one wave's packets in the order it decodes them, as dict(long, mapping, entries, bad)."""
    good = lambda v: not v["bad"]  # noqa: E731
    lds = lambda v: good(v) and 0 < v["entries"] <= 2048  # noqa: E731
    w3, w4 = _windows(visits, 3), _windows(visits, 4)
    assert any(all(map(good, w)) and [v["long"] for v in w] == [1, 0, 1] for w in w3), "long -> short -> long"
    assert any(all(map(good, w)) and [v["mapping"] for v in w] == [0, 2, 0] and all(v["long"] for v in w) for w in w3), "residue A -> B -> A"
    assert any(all(map(good, w)) and [v["mapping"] for v in w] == [0, 1, 0] for w in w3), "one submap -> two -> one"
    assert any(lds(w[0]) and good(w[1]) and w[1]["entries"] > 2048 and good(w[2]) and w[2]["entries"] == 0 and lds(w[3]) for w in w4), \
        "entries in LDS -> in global memory -> none -> in LDS"
    assert any(good(w[0]) and w[1]["bad"] and good(w[2]) for w in w3), "a flagged packet between two good ones"


@pytest.mark.parametrize("tables_in_lds", [False, True])
def test_every_wave_walks_a_tour_of_packets(tables_in_lds, capfd, monkeypatch):
    """A grid of 3 single-wave workgroups (tables in global memory) or of 2 workgroups of w waves (tables in LDS), 12 packets per
    wave: each wave decodes long, short, long, residue B, A, two submaps, A, a packet whose entries are read from global memory, one
    without entries, A, a packet with a bad mode (flagged by the layout kernel and skipped), A. Every packet but the flagged one is
    bit-exact; the status names the flagged one and nothing else."""
    grid = 2 if tables_in_lds else 3
    monkeypatch.setenv("VSYN_DEBUG", "1")
    monkeypatch.setenv("VSYN_VQ_GRID", str(grid))
    spec, vqs = vq_cases.walk_case(tables_in_lds)
    syn = Synth(spec, max_streams=4)
    g, w, lds, home = _attach(syn, vqs, capfd)
    assert g == grid and home == tables_in_lds and (w == 1 or tables_in_lds), (g, w, home)
    if tables_in_lds:
        assert lds <= 156 * 1024 and w >= 2, (w, lds)
    U = g * w  # waves; wave u decodes packets u, u + U, ...
    rng = np.random.default_rng(12)
    tour = vq_cases.WALK_TOUR
    pkts = [vq_cases.walk_packet(spec, vqs, "LA" if kind == "BAD" else kind, rng) for kind in tour for _ in range(U)]
    bad = [t * U + u for t, kind in enumerate(tour) if kind == "BAD" for u in range(U)]
    b = assemble_vq_batch(spec, pkts, 4, bad_mode=set(bad))
    for u in range(U):
        _assert_transitions([dict(long=pkts[p]["long"], mapping=pkts[p]["mapping"], entries=pkts[p]["ent"].size, bad=p in bad)
                             for p in range(u, len(pkts), U)])
    want = _expected(spec, vqs, pkts)
    out = _submit(syn, b)
    assert out["rc"] == VSYN_ERR_STREAM and out["flags"] == VSYN_ST_BAD_MODE and out["first_bad"] == bad[0], out
    _assert_bits(out, b, want, skip=set(bad))


def test_reattach_between_table_homes(capfd, monkeypatch):
    """One handle: a setup whose tables live in LDS, then one that keeps them in global memory, then the first again; each exact
    (against oracle and model) with the PCM behind it."""
    monkeypatch.setenv("VSYN_DEBUG", "1")
    spec, in_lds = vq_cases.walk_case(True)
    _, in_global = vq_cases.walk_case(False)
    syn = Synth(spec, max_streams=4)
    rng = np.random.default_rng(5)
    kinds = ["LA", "LB", "SA", "LBC", "BIG", "LA", "ZERO", "SA", "LBC", "LB"]
    for i, (vqs, home) in enumerate(((in_lds, True), (in_global, False), (in_lds, True))):
        assert _attach(syn, vqs, capfd)[3] == home
        pkts = [vq_cases.walk_packet(spec, vqs, kinds[(p + i) % len(kinds)], rng) for p in range(40)]
        b = assemble_vq_batch(spec, pkts, 4)
        want = _expected(spec, vqs, pkts, model=True)
        out = _submit(syn, b)
        assert out["rc"] == 0, (i, out)
        _assert_bits(out, b, want)
        _check_pcm(out, spec, b)


@pytest.fixture(scope="module")
def production_batch():
    """20 000 stereo 256/2048 packets tiled from 64 distinct ones (8 long, 56 short) in a fixed pseudo-random order, 40 streams."""
    spec = fixture_like_spec(2)
    vqs = synthetic_vq_spec(2, spec.blocksize1)
    rng = np.random.default_rng(2024)
    pool = [vq_pool_packet(spec, vqs, 1 if i < 8 else 0, random_own_mask(rng, 2), rng) for i in range(64)]
    pkts = [pool[i] for i in rng.integers(0, 64, 20000)]
    b = assemble_vq_batch(spec, pkts, 40)
    sizes = np.array([2 * k["n2"] for k in pkts], np.int64).reshape(40, 500)
    emitted = (sizes[:, :-1] // 4 + sizes[:, 1:] // 4).sum(axis=1)
    b["plane_stride"] = int(emitted.max()) + 64
    return spec, vqs, b, np.concatenate(_expected(spec, vqs, pkts))


@pytest.mark.parametrize("tables_in_lds", [True, False])
def test_production_launch_shape_walks_packets(tables_in_lds, production_batch, capfd, monkeypatch):
    """No knob: the grid is what the handle plans. With at most 10 000 waves resident (asserted from the launch line, not assumed)
    and 20 000 packets every wave decodes at least two. The residue buffer is not dirtied here (35 MB)."""
    monkeypatch.setenv("VSYN_DEBUG", "1")
    if not tables_in_lds:
        monkeypatch.setenv("VSYN_VQ_NO_LDS_TABLES", "1")
    spec, vqs, b, want = production_batch
    syn = Synth(spec, max_streams=40)
    g, w, _, home = _attach(syn, vqs, capfd)
    assert home == tables_in_lds
    assert g * w <= 10000, "%d workgroups x %d waves are resident: 20 000 packets do not make every wave walk two" % (g, w)
    out = _submit(syn, b, dirty=False)
    assert out["rc"] == 0, (out["rc"], out["flags"], out["first_bad"])
    assert np.array_equal(out["residue"].view(np.uint32), want.view(np.uint32))
    assert int(out["emit_len"].reshape(40, 500).sum(axis=1).max()) + 64 == b["plane_stride"]


# ---- d. entry staging ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables_in_lds", [True, False])
def test_entry_counts_around_the_staging_buffer(tables_in_lds, capfd, monkeypatch):
    """Packets of exactly 2044, 2048 (the most that is staged in LDS) and 2052 entries (read from global memory), each starting 0, 1
    and 7 entries behind a 16-byte boundary: 2048 entries at shift 7 fill the staging buffer to its last element. One workgroup, so
    the next packet of the same wave follows in the same LDS - its classes read the pass masks that lie behind that buffer."""
    monkeypatch.setenv("VSYN_DEBUG", "1")
    monkeypatch.setenv("VSYN_VQ_GRID", "1")
    if not tables_in_lds:
        monkeypatch.setenv("VSYN_VQ_NO_LDS_TABLES", "1")
    spec = fixture_like_spec(2)
    vqs = synthetic_vq_spec(2, spec.blocksize1)
    syn = Synth(spec, max_streams=1)
    g, U, _, home = _attach(syn, vqs, capfd)
    assert g == 1 and home == tables_in_lds
    rng = np.random.default_rng(9)
    special = [(n, shift) for n in vq_cases.STAGING_COUNTS for shift in (0, 1, 7)]
    pkts, mod8, at = [], [], {}
    for lo in range(0, len(special), U):
        row = special[lo:lo + U]
        for n, shift in row:
            at[(n, shift)] = len(pkts)
            pkts.append(vq_pool_packet(spec, vqs, 1, 3, rng, [vq_cases.staging_classes(vq_cases.STAGING_COUNTS[n], rng)]))
            mod8.append(shift)
        for _ in range(2 * U - len(row)):  # the rest of the row, then a row of followers: random classes, all of them in use
            pkts.append(vq_pool_packet(spec, vqs, 1, 3, rng))
            mod8.append(-1)
    b = assemble_vq_batch(spec, pkts, 1, ent_mod8=mod8)
    for (n, shift), p in at.items():
        assert b["vq_packets"]["num_entries"][p] == n and b["vq_packets"]["entry_off"][p] % 8 == shift
        assert p + U < len(pkts) and pkts[p + U]["ent"].size and len(set(pkts[p + U]["cls"])) >= 8  # its follower in the same wave
    want = _expected(spec, vqs, pkts)
    out = _submit(syn, b)
    assert out["rc"] == 0, out
    _assert_bits(out, b, want)


# ---- e. packed counts near 16 bits ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("psize,fmt", [(64, 2), (60, 2), (64, 1)])
def test_pass_counts_near_the_16_bit_halves(psize, fmt, capfd, monkeypatch):
    """15 channels at 8192/8192 in one format 2 vector of 61 440 elements: passes 0 and 1 hold 61 440 entries each (both halves of
    one packed scan word), pass 2 another 30 720. Partition 64: 960 partitions, the fast routes; partition 60: 1024 partitions (8192
    slots) through the general route with its tails. Format 1: the same counts from 15 vectors of 4096 side by side (a pass holds
    the entries of every vector of the submap)."""
    monkeypatch.setenv("VSYN_DEBUG", "1")
    spec, vqs = vq_cases.packed_counts_case(15, psize, fmt)
    rng = np.random.default_rng(psize)
    pkts = [vq_pool_packet(spec, vqs, mode, (1 << 15) - 1, rng) for mode in (1, 0)]
    assert all(k["ent"].size == 61440 * 2 + 30720 for k in pkts)
    syn = Synth(spec, max_streams=1)
    _attach(syn, vqs, capfd)  # accepted
    b = assemble_vq_batch(spec, pkts, 1)
    want = _expected(spec, vqs, pkts, model=psize == 64)
    out = _submit(syn, b)
    assert out["rc"] == 0, (out["rc"], out["flags"], out["first_bad"])
    _assert_bits(out, b, want)
    if psize == 64:
        _check_pcm(out, spec, b)


@pytest.mark.parametrize("fmt", [2, 1])
def test_sixteen_channels_of_8192_are_refused(fmt):
    """One channel more: 65 536 elements in the format 2 vector, or 65 536 entries in one pass of 16 format 1 vectors (the slot count,
    8192, and the vector length, 4096, are within the limits there) - neither fits the scan's 16-bit halves."""
    spec, vqs = vq_cases.packed_counts_case(16, 64, fmt)
    syn = Synth(spec, max_streams=1)
    with pytest.raises(VsynError, match="65535"):
        syn.attach_vq(vqs)


# ---- f. device entry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["synthetic", "5.1"])
def test_submit_device_vq_on_offset_buffers(name, capfd, monkeypatch):
    """vsyn_submit_device_vq (what the benchmark times) on torch buffers: the entry numbers start 3 elements into their allocation,
    the classifications at an odd byte. Residue and emit_len bit for bit what vsyn_submit_host_vq returns, status clean."""
    import torch
    monkeypatch.setenv("VSYN_DEBUG", "1")
    if name == "synthetic":
        spec = fixture_like_spec(2)
        vqs = synthetic_vq_spec(2, spec.blocksize1)
    else:
        spec, vqs = vq_cases.channel_case(name)
    S, per = 4, 10
    pkts = _random_packets(spec, vqs, S, per, [1, 1, 0, 1, 0], seed=61)
    syn = Synth(spec, max_streams=S)
    _attach(syn, vqs, capfd)
    b = assemble_vq_batch(spec, pkts, S)
    P, total = len(pkts), int(b["res_off"][-1])
    host = _submit(syn, b)
    assert host["rc"] == 0
    _assert_bits(host, b, _expected(spec, vqs, pkts))
    dev = "cuda"
    ent_store = torch.zeros(b["entries"].size + 3 + 16, dtype=torch.int16, device=dev)
    ent = ent_store[3:3 + b["entries"].size]
    ent.copy_(torch.from_numpy(b["entries"].view(np.int16)))
    cls_store = torch.zeros(b["cls"].size + 1 + 16, dtype=torch.uint8, device=dev)
    cls = cls_store[1:1 + b["cls"].size]
    cls.copy_(torch.from_numpy(b["cls"]))
    assert ent.data_ptr() % 16 == 6 and cls.data_ptr() % 2 == 1
    d = dict(pk=torch.from_numpy(b["packets"].view(np.uint8)).to(dev), seg=torch.from_numpy(b["segments"].view(np.uint8)).to(dev),
             ys=torch.from_numpy(host["ys"].astype(np.int16)).to(dev), vqp=torch.from_numpy(b["vq_packets"].view(np.uint8)).to(dev),
             res=torch.full((total,), DIRT, device=dev), pcm=torch.zeros((S, spec.channels, b["plane_stride"]), device=dev),
             emit=torch.zeros(P, dtype=torch.int32, device=dev))
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    syn.reset()
    syn.submit_device_vq(P, d["pk"].data_ptr(), S, d["seg"].data_ptr(), per, d["ys"].data_ptr(), d["vqp"].data_ptr(), cls.data_ptr(),
                         b["cls"].size, ent.data_ptr(), b["entries"].size, d["res"].data_ptr(), d["pcm"].data_ptr(), b["plane_stride"],
                         d["emit"].data_ptr(), 0, stream)
    fl, bad = syn.sync_status(stream)
    assert fl == 0, (fl, bad)
    assert np.array_equal(d["res"].cpu().numpy().view(np.uint32), host["residue"].view(np.uint32))
    assert np.array_equal(d["emit"].cpu().numpy().astype(np.uint32), host["emit_len"])


# ---- g. status from a later visit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["entry", "class"])
@pytest.mark.parametrize("tables_in_lds", [False, True])
def test_bad_number_on_a_waves_third_visit(tables_in_lds, what, capfd, monkeypatch):
    """An entry number beyond its book, or a classification beyond the residue's classes, in the packet that is one wave's third
    visit: VSYN_ERR_STREAM, VSYN_ST_BAD_VQ and first_bad_packet name it, and the next clean submit is exact. Malformed data the stage
    is specified to flag; numbers stay inside uint16 and offsets inside the arrays. include/vorbis_synth_hip.h does not say what the
    OTHER packets of a flagged submit hold, so that is not asserted."""
    grid = 2 if tables_in_lds else 3
    monkeypatch.setenv("VSYN_DEBUG", "1")
    monkeypatch.setenv("VSYN_VQ_GRID", str(grid))
    spec, vqs = vq_cases.walk_case(tables_in_lds)
    syn = Synth(spec, max_streams=1)
    g, w, _, home = _attach(syn, vqs, capfd)
    assert g == grid and home == tables_in_lds
    U = g * w
    rng = np.random.default_rng(3)
    pkts = [vq_cases.walk_packet(spec, vqs, "LA", rng) for _ in range(4 * U)]
    b = assemble_vq_batch(spec, pkts, 1)
    victim = 2 * U + 1  # wave 1: packets 1, U + 1, 2 U + 1
    spoiled = dict(b)
    if what == "entry":
        spoiled["entries"] = b["entries"].copy()
        spoiled["entries"][int(b["vq_packets"]["entry_off"][victim])] = 65535
    else:
        spoiled["cls"] = b["cls"].copy()
        spoiled["cls"][int(b["vq_packets"]["cls_off"][victim]) + 1] = 200
    out = _submit(syn, spoiled)
    assert out["rc"] == VSYN_ERR_STREAM and out["flags"] == VSYN_ST_BAD_VQ and out["first_bad"] == victim, out
    out = _submit(syn, b)
    assert out["rc"] == 0, out
    _assert_bits(out, b, _expected(spec, vqs, pkts))
