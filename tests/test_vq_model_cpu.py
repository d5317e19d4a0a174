"""CPU: tests/vq_model.py (residue decode written from Vorbis I 8.6.2 - 8.6.5) against the oracle's residue_vq, bit for bit, on
every setup of tests/vq_cases.py and on both fixtures' real entry streams (where the oracle is itself pinned to the reference's
'after_residue', tests/test_host_decoder.py). The GPU tests compare the kernel with the oracle; this file is what makes the oracle
a judge for the shapes that no reference stream has: more than two channels per submap, format 0 / 1 submaps of several channels,
every block size."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
from oracle import oracle_binding as ob
from tests import vq_cases, vq_model
from tests.workloads import (GOLDEN, build_probe, load_golden, propagated_used, read_entropy_dump, synth_vq_packet, vq_pool_packet,
                             vq_submap_shapes)

CASES = vq_cases.all_cases()


def _same(spec, vqs, k):
    rc, want = ob.residue_vq(vqs, k["mapping"], spec.channels, k["n2"], k["used"], k["cls"], k["ent"])
    assert rc == 0
    got = vq_model.residue_vq(vqs, k["mapping"], spec.channels, k["n2"], k["used"], k["cls"], k["ent"])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return want


def _masks(spec):
    """all used, none used, and partial masks that the coupling step changes (where the setup has couplings) or leaves alone"""
    C = spec.channels
    out = [(1 << C) - 1, 0, 1 << (C - 1), 1]
    if C > 2:
        out.append(0b101 if C == 3 else (1 << C) - 1 - 0b110)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_matches_oracle_on_every_setup(name):
    """A few random packets per mode and per mask; some value must be non-zero and (where a class has two passes) the sums must
    round, or bit equality would say nothing about the order of the additions."""
    spec, vqs = CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    big = name.startswith("packed/")
    nonzero = inexact = 0
    for mode in range(len(spec.modes)):
        if big and mode == 0:
            continue  # (both modes are the same 8192 block; one packet of 150 000 entries is enough on the CPU)
        for own in (_masks(spec)[:1] if big else _masks(spec)):
            k = vq_pool_packet(spec, vqs, mode, own, rng)
            want = _same(spec, vqs, k)
            nonzero += int(np.count_nonzero(want))
            inexact += int(np.count_nonzero(want != np.round(want * 4) / 4))
            if own == 0 and all(r["type"] != 2 for r in vqs.residues):
                assert k["ent"].size == 0 and not want.any()
    assert nonzero and inexact


def test_format2_cases_miss_the_channel_count():
    """The format 2 setups of section a: begin and the end of the last partition are no multiples of the channel count on long blocks."""
    for name in ("f2x3", "f2x5", "f2x6"):
        spec, vqs = vq_cases.channel_case(name)
        r = vqs.residues[0]
        (_, parts), = vq_submap_shapes(vqs, 1, spec.channels, spec.blocksize1 // 2)
        assert r["begin"] % spec.channels and (r["begin"] + parts * r["partition_size"]) % spec.channels, name
        assert 8 * parts <= 8192


def test_chained_coupling_mask():
    spec, _ = vq_cases.channel_case("chain3")
    assert propagated_used(spec, 1, 0b100) == 0b110 and propagated_used(spec, 1, 0b001) == 0b111


def test_chosen_classes_give_exact_entry_counts():
    """synth_vq_packet with chosen classifications: the entry counts the staging tests rely on."""
    from tests.workloads import synthetic_vq_spec
    vqs = synthetic_vq_spec(2, 2048)
    r = vqs.residues[0]
    cost = []
    for c in range(10):
        cost.append(sum(32 // vqs.codebooks[b][0] for b in r["books"][c * 8:c * 8 + 8] if b >= 0))
    assert cost == [0, 4, 24, 8, 48, 16, 56, 32, 36, 56]
    rng = np.random.default_rng(1)
    for total, counts in vq_cases.STAGING_COUNTS.items():
        cls = vq_cases.staging_classes(counts, rng)
        c, e = synth_vq_packet(vqs, 1, 2, 1024, 3, rng, [cls])
        assert e.size == total and c.size == 50
    # unchanged for callers that pass no classes: same draws as before this argument existed
    a = synth_vq_packet(vqs, 1, 2, 1024, 3, np.random.default_rng(5))
    b = synth_vq_packet(vqs, 1, 2, 1024, 3, np.random.default_rng(5), None)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    entry.build_hip()
    entry.build_host()
    return build_probe(tmp_path_factory.mktemp("probe"))


@pytest.mark.parametrize("name", ["test.stereo44khz", "test.mono44khz"])
def test_model_rebuilds_reference_residue(probe, name, tmp_path):
    """The fixtures' real classifications and entry numbers (the host decoder's dump): the model rebuilds the reference decoder's
    'after_residue' of every packet, bit for bit - as the oracle does (tests/test_host_decoder.py)."""
    spec, b, _ = load_golden(name)
    out = str(tmp_path / "e.bin")
    r = subprocess.run([probe, os.path.join(GOLDEN, name + ".ogg"), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    d = read_entropy_dump(out)
    Cn = spec.channels
    off = 0
    for p in range(d["P"]):
        mode = int(d["packets"]["mode"][p])
        n2 = spec.blocksize_of_mode(mode) // 2
        vp = d["vq_packets"][p]
        c0 = int(vp["cls_off"])
        c1 = int(d["vq_packets"][p + 1]["cls_off"]) if p + 1 < d["P"] else d["cls"].size
        e0, ne = int(vp["entry_off"]), int(vp["num_entries"])
        used = propagated_used(spec, mode, int(d["packets"]["floor_used"][p]))
        got = vq_model.residue_vq(d["vq_spec"], spec.modes[mode][1], Cn, n2, used, d["cls"][c0:c1], d["entries"][e0:e0 + ne])
        want = b["residue"][off:off + Cn * n2]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), p
        off += Cn * n2
    assert off == b["residue"].size


def test_model_refuses_what_does_not_describe_a_packet():
    spec, vqs = vq_cases.channel_case("f1x3")
    k = vq_pool_packet(spec, vqs, 1, 7, np.random.default_rng(2))
    with pytest.raises(vq_model.BadStream):
        vq_model.residue_vq(vqs, 1, 3, k["n2"], 7, k["cls"], k["ent"][:-1])
    with pytest.raises(vq_model.BadStream):
        vq_model.residue_vq(vqs, 1, 3, k["n2"], 7, k["cls"], np.append(k["ent"], 0).astype(np.uint16))
