"""GPU: the damaged files of tests/golden/damaged.npz (oracle/make_damaged_goldens.py) on every decode path, against the oracle,
which tests/test_damaged_files.py pins to the REFERENCE decoder bit for bit on the same records:
  a. direct: the entropy half's output (the complete packets in front of a read error) through Synth.submit_host on each of the
     preparation kernel, the chained pre-kernels and the staged kernels (and the ring mode of the tuned kernel where the run plan
     has one) — status code, failing packet and emit_len in front of it exact, the oracle's status flag among the device's, PCM
     within the suite's gate; the kernels that ran read back from the library's kernel profile;
  b. batched: the accepted files of one setup in one submit (one segment each, sharing workgroups, runs and ring groups), with the
     library's run length and with VSYN_RUN_LEN=3 — each segment bit-identical to its single-file submit;
  c. end to end: the corpus decoder over all records in mixed batches, float residue and VQ: verdicts, frame counts, PCM, and
     every file bit-identical to its decode in a submit of its own;
  d. the CLI (ours_hip.bin --debug_out): exit status, hook stream and delivered PCM."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

from oracle import oracle_binding as ob
from parseoggvorbis_amd import binding
from tests.dump_reader import read_dump
from tests.test_damaged_files import entropy_prefix
from tests.test_gpu_host_decoder import CLI, _run_corpus
from tests.test_gpu_parity import PATHS
from tests.workloads import build_probe, damaged_bytes, fixture_setup, load_damaged

pytestmark = pytest.mark.gpu
RECORDS, Z = load_damaged()
GATE = 1e-5


def gate(want):
    return GATE * max(1.0, float(np.abs(want).max()) if want.size else 0.0)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """per record: (record, setup, entropy dump or None, oracle result or None, oracle PCM [C, frames]); one probe build"""
    td = tmp_path_factory.mktemp("damaged")
    probe = build_probe(td)
    specs, out = {}, []
    for rec in RECORDS:
        spec = specs.setdefault(rec["base"], fixture_setup(rec["base"]))
        data = damaged_bytes(rec)
        _, d = entropy_prefix(probe, data, td)
        res = pcm = None
        if d is not None and d["P"]:
            res = _submit(ob.OracleSynth(spec, 1), spec, d)
            frames = int(res["emit_len"].sum())
            assert frames == rec["ref_frames"], rec["index"]
            pcm = res["pcm"][0][:, :frames]
        out.append(dict(rec=rec, spec=spec, d=d, res=res, pcm=pcm, data=data))
    return out


def _seg(P):
    seg = np.zeros(1, binding.SEGMENT_DTYPE)
    seg["num_packets"], seg["flags"] = P, binding.VSYN_SEG_RESET
    return seg


def _plane(spec, P):
    return P * (spec.blocksize1 // 2) + 64


def _submit(synth, spec, d, **kw):
    return synth.submit_host(d["packets"], _seg(d["P"]), d["ys"], d["residue"], _plane(spec, d["P"]), **kw)


RING_RUN_LEN = 4


def ring_planned(spec, d, R=RING_RUN_LEN):
    """Whether the fused long-block kernel takes a workgroup of this one-segment stereo submit in ring mode at run length R
    (vsyn_fused.h, fused_kernel_body: the 8 runs x 2 channels of the workgroup lie in the segment and every run is class 1 —
    run_class: its packets and its one-packet halo are valid long blocks)"""
    if spec.channels != 2:
        return False
    lg = np.asarray([int(m) < len(spec.modes) and spec.modes[int(m)][0] for m in d["packets"]["mode"]], bool)
    runs = (d["P"] + R - 1) // R
    for b in range(runs // 8):
        lo, hi = max(0, 8 * b * R - 1), min(d["P"], (8 * b + 8) * R)
        if lg[lo:hi].all():
            return True
    return False


def _check(got, want, c, ctx):
    # (the flag word may hold more bits than the oracle's, which stops at the first failure: vsyn_staged.h, pkt_step_core)
    assert (got["rc"], got["first_bad"]) == (want["rc"], want["first_bad"]), (ctx, got["flags"], want["flags"])
    assert got["flags"] & want["flags"] == want["flags"] and (want["rc"] or got["flags"] == 0), (ctx, got["flags"], want["flags"])
    # (the device goes on checking the packets behind a refused one, the oracle stops there: emit_len in front of it)
    upto = c["d"]["P"] if want["rc"] == 0 else int(want["first_bad"])
    assert np.array_equal(got["emit_len"][:upto], want["emit_len"][:upto]), ctx
    frames = c["pcm"].shape[1]
    err = float(np.abs(got["pcm"][0][:, :frames] - c["pcm"]).max()) if frames else 0.0
    assert err <= gate(c["pcm"]), (ctx, err)
    return err / max(1.0, float(np.abs(c["pcm"]).max()) if frames else 1.0)


def test_direct_submit_on_every_path(cases, monkeypatch):
    """Every record through each preparation path. Which synthesis kernel ran is read back from the library's kernel profile: the
    tuned 256/2048 kernel or the size-generic fused kernel on the fused paths, a staged kernel under VSYN_SUBMIT_STAGED (every
    committed setup gets a fused kernel of its own choice, so the staged kernels run on that path only). Records whose run plan
    holds a ring-mode workgroup are submitted once more at that run length."""
    gpus, rings, worst = {}, {}, {f: 0.0 for f in PATHS + ["ring"]}
    reached = dict(vsyn_fused_kernel=0, vsyn_fused_u_kernel=0, staged=0, ring=0)
    for c in cases:
        rec, spec, d, want = c["rec"], c["spec"], c["d"], c["res"]
        if want is None:
            continue
        g = gpus.get(rec["base"])
        if g is None:
            g = gpus[rec["base"]] = binding.Synth(spec, device=0, max_streams=1)
            g.profile(1)
        fp = g.fused_paths & 0xff
        for flags in PATHS:
            g.reset()
            got = _submit(g, spec, d, flags=flags)
            _, launches, kernel = g.profile_read()
            ctx = (rec["index"], rec["base"], flags, fp, launches, kernel)
            if flags == binding.VSYN_SUBMIT_STAGED:
                assert launches and "staged" in kernel, ctx
                reached["staged"] += 1
            elif launches:
                reached[kernel] = reached.get(kernel, 0) + 1
            worst[flags] = max(worst[flags], _check(got, want, c, ctx))
        if (fp & 1) and ring_planned(spec, d):
            r = rings.get(rec["base"])
            if r is None:
                monkeypatch.setenv("VSYN_RUN_LEN", str(RING_RUN_LEN))
                r = rings[rec["base"]] = binding.Synth(spec, device=0, max_streams=1)
                monkeypatch.delenv("VSYN_RUN_LEN")
            r.reset()
            worst["ring"] = max(worst["ring"], _check(_submit(r, spec, d), want, c, (rec["index"], rec["base"], "ring")))
            reached["ring"] += 1
    print("kernels reached (records): %s; worst error / max(1, peak) per path %s" % (reached, worst))
    print("fused_paths per setup: %s" % {b: g.fused_paths for b, g in gpus.items()})
    for g in list(gpus.values()) + list(rings.values()):
        g.close()
    assert all(reached.values()), reached


def _concat(spec, ds):
    pk = np.concatenate([d["packets"] for d in ds])
    ys = np.concatenate([d["ys"] for d in ds])
    res = np.concatenate([d["residue"] for d in ds])
    segs = np.zeros(len(ds), binding.SEGMENT_DTYPE)
    first = roff = 0
    for i, d in enumerate(ds):
        segs[i] = (i, first, d["P"], binding.VSYN_SEG_RESET, roff)
        first += d["P"]
        roff += len(d["residue"])
    return pk, segs, ys, res, _plane(spec, max(d["P"] for d in ds))


@pytest.mark.parametrize("run_len", [0, 3])
def test_batched_damaged_streams_equal_single_submits(cases, run_len, monkeypatch):
    by_base = {}
    for c in cases:
        if c["rec"]["expect_ok"] and c["res"] is not None:
            by_base.setdefault(c["rec"]["base"], []).append(c)
    for base, cs in by_base.items():
        spec = cs[0]["spec"]
        if run_len:
            monkeypatch.setenv("VSYN_RUN_LEN", str(run_len))
        else:
            monkeypatch.delenv("VSYN_RUN_LEN", raising=False)
        single = []
        g1 = binding.Synth(spec, device=0, max_streams=1)
        for c in cs:
            g1.reset()
            single.append(_submit(g1, spec, c["d"]))
        g1.close()
        pk, segs, ys, res, plane = _concat(spec, [c["d"] for c in cs])
        g = binding.Synth(spec, device=0, max_streams=len(cs))
        got = g.submit_host(pk, segs, ys, res, plane)
        g.close()
        monkeypatch.delenv("VSYN_RUN_LEN", raising=False)
        assert got["rc"] == 0, (base, got["rc"], got["flags"])
        for i, (c, one) in enumerate(zip(cs, single)):
            a, n = int(segs[i]["first_packet"]), int(segs[i]["num_packets"])
            assert np.array_equal(got["emit_len"][a:a + n], one["emit_len"]), (base, i)
            frames = int(one["emit_len"].sum())
            assert frames == c["rec"]["ref_frames"]
            assert np.array_equal(got["pcm"][i][:, :frames].view(np.uint32), one["pcm"][0][:, :frames].view(np.uint32)), (base, i)


@pytest.mark.parametrize("vq", ["0", "1"])
def test_corpus_decoder_on_damaged_files(cases, vq, monkeypatch):
    """All records in mixed batches: verdicts, frame counts and PCM as expected; a refused file fails alone — every file decodes to
    the same bits as in a submit of its own."""
    monkeypatch.setenv("PARSEOGGVORBIS_VQ", vq)
    blobs = [c["data"] for c in cases]
    chans = [c["spec"].channels for c in cases]
    frames, _, ok, pcm, _ = _run_corpus(blobs, chans, threads=4, feeders=2, files_per_submit=8)
    frames1, _, ok1, pcm1, _ = _run_corpus(blobs, chans, threads=4, feeders=2, files_per_submit=1)
    bad = []
    for i, c in enumerate(cases):
        rec = c["rec"]
        # A file the entropy half refuses delivers the packets in front of the failure, as the reference does (CorpusDecoder::take).
        # A file the GPU refuses (its status flags) delivers no PCM at all (CorpusDecoder::deliver): the corpus API hands out a
        # file's PCM from a submit it was accepted in; the CLI delivers that prefix (test_cli_on_damaged_files).
        want = rec["ref_frames"] if rec["expect_ok"] or rec["expect_flags"] == 0 else 0
        if bool(ok[i]) != rec["expect_ok"] or frames[i] != want:
            bad.append((rec["index"], rec["base"], "verdict/frames", ok[i], frames[i], rec["expect_ok"], rec["expect_flags"], want))
            continue
        n = frames[i]
        if n and float(np.abs(pcm[i][:, :n] - c["pcm"]).max()) > gate(c["pcm"]):
            bad.append((rec["index"], rec["base"], "pcm"))
        if (ok1[i], frames1[i]) != (ok[i], frames[i]) or not np.array_equal(pcm1[i][:, :n].view(np.uint32), pcm[i][:, :n].view(np.uint32)):
            bad.append((rec["index"], rec["base"], "neighbours"))
    assert not bad, bad


def _hook_digest(entries, upto):
    """The CLI dump's non-PCM hooks of audio packets [0, upto) in the digest form of make_damaged_goldens.hook_stream"""
    import hashlib
    h = hashlib.sha256()
    sums, abss = [], []
    pk = -1
    for nm, ch, v, _ in entries:
        if nm == "start_audio_packet":
            pk += 1
        if pk >= upto:
            break
        if nm == "pcm":
            continue
        f = v.dtype.kind == "f"
        h.update(("%s|%d|%d|%d|%d;" % (nm, ch, len(v), f, 0 if f else zlib.crc32(v.astype(np.int64).tobytes()))).encode())
        sums.append(float(v.astype(np.float64).sum()) if f else 0.0)
        abss.append(float(np.abs(v.astype(np.float64)).sum()) if f else 0.0)
    return h.hexdigest(), np.asarray(sums), np.asarray(abss)


def test_cli_on_damaged_files(cases, tmp_path):
    """ours_hip.bin --debug_out on every refused record and on the accepted ones the generator stored hooks for: the exit status of
    the expected verdict, the reference's hook stream (integers exact, floats to 1e-5 of their magnitude sums), and the PCM it
    delivered — the reference's frame count, within the gate of the oracle's."""
    ran = 0
    for c in cases:
        rec = c["rec"]
        if not rec["hook_num"]:
            continue
        ran += 1
        src, dump = str(tmp_path / "d.ogg"), str(tmp_path / "d.bin")
        open(src, "wb").write(c["data"])
        r = subprocess.run(["timeout", "-k", "10", "60", CLI, "--in", src, "--debug_out", dump], capture_output=True, text=True)
        ctx = (rec["index"], rec["base"], rec["kind"], r.returncode, r.stderr[-300:])
        assert r.returncode == (0 if rec["expect_ok"] else 1), ctx
        header, entries = read_dump(dump)
        upto = 1 << 30 if rec["expect_ok"] else rec["expect_bad"]
        sha, sums, abss = _hook_digest(entries, upto)
        o, n = rec["hook_off"], rec["hook_num"]
        assert sha == rec["hook_sha"] and len(sums) == n, ctx
        ws, wa = Z["hook_sum"][o:o + n], Z["hook_abs"][o:o + n]
        tol = 1e-5 * (wa + 1e-30) + 1e-12
        assert (np.abs(sums - ws) <= tol).all() and (np.abs(abss - wa) <= tol).all(), ctx
        Cn = c["spec"].channels
        pcm = [np.concatenate([v for nm, ch, v, _ in entries if nm == "pcm" and ch == k] or [np.zeros(0, np.float32)]) for k in range(Cn)]
        for k in range(Cn):
            assert len(pcm[k]) == rec["ref_frames"], ctx
            if rec["ref_frames"]:
                assert np.abs(pcm[k] - c["pcm"][k]).max() <= gate(c["pcm"]), ctx
    assert ran >= 90
