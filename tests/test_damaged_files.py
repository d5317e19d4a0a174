"""Damaged files (tests/golden/damaged.npz, oracle/make_damaged_goldens.py: bit flips, overwritten bytes, moved granules, header-type
bits and truncation over the committed fixtures, page CRCs recomputed) against the REFERENCE decoder's verdict, hooks and PCM, on the
CPU: the host entropy half (tests/host_entropy_dump.cpp --prefix) and the oracle behind it must reproduce what the reference did —
accept what it accepts with the same PCM bit for bit, stop where it stops with the same PCM in front of the failure, and refuse
class A by name at its packet."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle_binding as ob
from parseoggvorbis_amd import binding
from tests.workloads import (build_probe, damaged_bytes, entropy_hook_digests, fixture_setup, load_damaged, read_entropy_dump,
                             sha256_bits)

RECORDS, _ = load_damaged()


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    import __graft_entry__ as entry
    entry.build_hip()
    entry.build_host()
    return build_probe(tmp_path_factory.mktemp("probe"))


def entropy_prefix(probe, data, tmp_path, vq="0"):
    """-> (probe exit status, entropy dump or None): 0 the whole stream, 4 the complete packets in front of a read error,
    5 a read error before any audio packet, 6 a stream without audio packets"""
    src, out = str(tmp_path / "d.ogg"), str(tmp_path / "e.bin")
    open(src, "wb").write(data)
    r = subprocess.run(["timeout", "-k", "10", "60", probe, "--prefix", src, out], capture_output=True, text=True,
                       env=dict(os.environ, PARSEOGGVORBIS_VQ=vq))
    assert r.returncode in (0, 4, 5, 6), (r.returncode, r.stdout[-300:], r.stderr[-300:])
    return r.returncode, (read_entropy_dump(out) if r.returncode in (0, 4) else None)


def oracle_decode(spec, d):
    """The oracle's synthesis of every packet of an entropy dump, one segment -> submit_host result"""
    seg = np.zeros(1, binding.SEGMENT_DTYPE)
    seg["num_packets"], seg["flags"] = d["P"], binding.VSYN_SEG_RESET
    plane = d["P"] * (spec.blocksize1 // 2) + 64
    return ob.OracleSynth(spec, max_streams=1).submit_host(d["packets"], seg, d["ys"], d["residue"], plane)


def check_verdict(rec, status, d):
    """The entropy half stops where the reference's entropy half stops; it passes every packet the synthesis half refuses."""
    P = d["P"] if d is not None else 0
    if rec["expect_ok"]:  # (6: truncated in front of the first audio page, which the reference accepts too)
        assert status == 0 or (status == 6 and rec["ref_packets"] == 0), status
    elif rec["expect_flags"] == 0:  # refused by the entropy half: exactly the packets in front of the failing one
        assert status in (4, 5) and P == rec["expect_bad"], (status, P, rec["expect_bad"], rec["ref_err"])
    else:
        assert P > rec["expect_bad"], (status, P, rec["expect_bad"])


def check_oracle(rec, res):
    if rec["expect_ok"] or rec["expect_flags"] == 0:
        assert (res["rc"], res["flags"]) == (0, 0), (res["rc"], res["flags"])
    else:
        assert (res["rc"], res["flags"], res["first_bad"]) == (binding.VSYN_ERR_STREAM, rec["expect_flags"], rec["expect_bad"]), \
            (res["rc"], res["flags"], res["first_bad"], rec["expect_flags"], rec["expect_bad"], rec["ref_err"])
    frames = int(res["emit_len"].sum())
    assert frames == rec["ref_frames"], (frames, rec["ref_frames"])
    assert sha256_bits(res["pcm"][0][:, :frames]) == rec["ref_pcm"]


def test_records_cover_the_quotas():
    """The committed records hold what the generator promises: every base fixture, every recipe kind, every verdict."""
    kinds = [r["kind"] for r in RECORDS]
    assert len(RECORDS) >= 190
    assert sum(r["expect_ok"] for r in RECORDS) >= 120
    assert sum(not r["expect_ok"] and r["expect_flags"] == 0 for r in RECORDS) >= 30
    assert sum(r["expect_flags"] in (binding.VSYN_ST_FLOOR_RANGE, binding.VSYN_ST_FLOOR_VALUE, binding.VSYN_ST_GRANULE)
               for r in RECORDS) >= 25
    assert kinds.count("b") >= 20 and kinds.count("d") >= 20 and set(kinds) == set("abcd")
    for name in {r["base"] for r in RECORDS}:
        assert sum(r["base"] == name for r in RECORDS) >= 5, name
    assert len({r["base"] for r in RECORDS}) == 19


def test_damaged_files_match_the_reference(probe, tmp_path):
    """For every record: the rebuilt bytes match their digest; the entropy half's floor1 ys and residue equal the reference's hooks
    (of the packets in front of the failure, for a refused file); the oracle's verdict is the expected one, and its PCM the
    reference's, bit for bit."""
    specs = {}
    for rec in RECORDS:
        ctx = (rec["index"], rec["base"], rec["kind"], rec["seed"], rec["draw"])
        spec = specs.setdefault(rec["base"], fixture_setup(rec["base"]))
        data = damaged_bytes(rec)
        status, d = entropy_prefix(probe, data, tmp_path)
        try:
            check_verdict(rec, status, d)
            if d is None:
                assert rec["ref_frames"] == 0 and rec["expect_bad"] in (-1, 0)
                continue
            upto = d["P"] if rec["expect_ok"] else rec["expect_bad"]
            assert entropy_hook_digests(spec, d, upto) == (rec["ref_ys"], rec["ref_res"])
            check_oracle(rec, oracle_decode(spec, d))
        except AssertionError as e:
            raise AssertionError("record %s: %s" % (ctx, e)) from e
