#!/usr/bin/env python3
"""Damaged Ogg files for differential tests against the REFERENCE decoder. TEST INFRASTRUCTURE (authoring container only, like
make_synth_ogg.py): needs oracle/_ref/ours.bin and oracle/_ref/ours_asan.bin (`make -C oracle _ref/ours.bin _ref/ours_asan.bin`).

Seeded damage recipes over the committed fixtures (test.stereo44khz, test.mono44khz, synth_00 ... synth_15, winflags_bcd); the
header pages stay intact, so every file keeps its base fixture's setup:

    a  1-3 bit flips or overwritten bytes in the audio pages
    b  the granule of a random audio page, or of the last page, moved by up to +-3000 or set to 0
    c  the header-type bits of an audio page
    d  truncation at a random byte past the headers

Every complete page's CRC is then recomputed (tests/workloads.py fix_page_crcs), so that the damage reaches the codec. A draw is
dropped when the file equals its base, when the ASan build of the reference reports a memory error, or when the reference aborts
(an assert inside it: no verdict to compare with). The reference decodes every other draw with --debug_out; about 200 records are
kept (quotas below) in ONE file, tests/golden/damaged.npz, which holds recipes and digests, no PCM:

    base, kind, edit_pos / edit_val (+ edit_off), trunc     the recipe (trunc -1: none)
    sha                                                     sha256 of the damaged bytes
    ref_rc, ref_err                                         the reference's exit status and the tail of its error text
    ref_packets, ref_frames                                 audio packets it started, PCM frames it delivered
    ref_pcm                                                 sha256 of the delivered PCM's float32 bits, [channels, ref_frames]
    ref_ys, ref_res                                         sha256 of its "floor1 ys" / "after_residue" hooks of the packets in
                                                            front of expect_bad (every packet of an accepted file), see
                                                            hook_digests
    hook_sha, hook_off, hook_num, hook_sum, hook_abs        the non-PCM hook stream of those packets in the digest form of
                                                            make_synth_ogg.py: sha256 over names, channels, lengths and the CRCs
                                                            of the integer hooks; sum and sum of magnitudes of each float hook
                                                            (records the CLI test runs only: hook_num 0 elsewhere)
    expect_ok, expect_flags, expect_bad                     the product's expected verdict: accept (expect_bad -1); refuse where the
                                                            reference refuses (flags 0: in the entropy half, before packet
                                                            expect_bad; VSYN_ST_FLOOR_RANGE / _FLOOR_VALUE / _GRANULE: in the
                                                            synthesis half, at packet expect_bad); or refuse with
                                                            VSYN_ST_WINDOW_FLAGS at packet expect_bad (class A, DESIGN.md §7: a long
                                                            block with next_long set in front of a short block, which the reference
                                                            accepts)

    python oracle/make_damaged_goldens.py
"""
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import read_dump  # noqa: E402
from tests.workloads import GOLDEN, fix_page_crcs, ogg_pages  # noqa: E402

BASES = ["test.stereo44khz", "test.mono44khz"] + ["synth_%02d" % i for i in range(16)] + ["winflags_bcd"]
SEEDS = range(1, 4)
DRAWS_PER_SEED = int(os.environ.get("DRAWS", 400))
TARGET = 200
QUOTA = dict(accepted=120, entropy=30, synthesis=25, per_base=5, kind_b=20, kind_d=20)
CLI_ACCEPTED = 20  # accepted records whose hook stream the CLI test compares (besides every refused one)
FLOOR_RANGE, FLOOR_VALUE, GRANULE, WINDOW_FLAGS = 1, 2, 4, 128
OURS = os.path.join(HERE, "_ref", "ours.bin")
ASAN = os.path.join(HERE, "_ref", "ours_asan.bin")


def synthesis_flag(err):
    """The product's status flag for a refusal in the reference's synthesis half, from its error text; 0: entropy half."""
    if "check failed: predicted <= range" in err:
        return FLOOR_RANGE
    if "check failed: floor[i] < 256" in err:
        return FLOOR_VALUE
    if "abs_total_pos" in err or ("ParseOggVorbis.hpp:10" in err and "check failed: false" in err):  # forwardReadyPcm
        return GRANULE
    return 0


def base_info(name):
    data = open(os.path.join(GOLDEN, name + ".ogg"), "rb").read()
    pages = ogg_pages(data)
    npk, audio = 0, None
    for i, (o, ln, ends) in enumerate(pages):
        npk += ends
        if npk >= 3:
            audio = pages[i + 1:]
            break
    if name.startswith("test."):
        blockflag = [0, 1]
    else:
        blockflag = [int(v) for v in np.load(os.path.join(GOLDEN, name + ".npz"))["mode_blockflag"]]
    return dict(name=name, data=data, audio=audio, audio_start=audio[0][0], blockflag=blockflag)


def draw(rng, info):
    """-> (kind, {pos: new byte}, trunc) of one recipe"""
    data, audio = info["data"], info["audio"]
    kind = "abcd"[int(rng.choice(4, p=[0.4, 0.25, 0.1, 0.25]))]
    edits, trunc = {}, -1
    if kind == "a":
        for _ in range(int(rng.integers(1, 4))):
            o, ln, _ = audio[int(rng.integers(0, len(audio)))]
            p = o + int(rng.integers(0, ln))
            if 22 <= p - o < 26:  # the CRC field is rewritten anyway
                p = o + 26
            cur = edits.get(p, data[p])
            edits[p] = cur ^ (1 << int(rng.integers(0, 8))) if rng.random() < 0.6 else int(rng.integers(0, 256))
    elif kind == "b":
        o = audio[-1][0] if rng.random() < 0.4 else audio[int(rng.integers(0, len(audio)))][0]
        g = int.from_bytes(data[o + 6:o + 14], "little", signed=True)
        g = 0 if rng.random() < 0.15 else g + int(rng.integers(-3000, 3001))
        for i, v in enumerate(int(g).to_bytes(8, "little", signed=True)):
            edits[o + 6 + i] = v
    elif kind == "c":
        o = audio[int(rng.integers(0, len(audio)))][0]
        edits[o + 5] = data[o + 5] ^ int(rng.integers(1, 8))
    else:
        trunc = int(rng.integers(info["audio_start"] + 1, len(data)))
    edits = {p: v for p, v in edits.items() if data[p] != v}
    return kind, edits, trunc


def apply(info, edits, trunc):
    b = bytearray(info["data"])
    for p, v in edits.items():
        b[p] = v
    if trunc >= 0:
        del b[trunc:]
    return bytes(fix_page_crcs(b))


def audio_packets(data):
    """The audio packets of the complete pages of data, in the reference's page walk (a packet never spans pages there)."""
    out, n = [], 0
    for o, ln, _ in ogg_pages(data):
        ns = data[o + 26]
        lace = data[o + 27:o + 27 + ns]
        p, cur = o + 27 + ns, 0
        for v in lace:
            cur += v
            if v < 255:
                if n >= 3:
                    out.append(data[p:p + cur])
                p += cur
                cur = 0
                n += 1
    return out


def window_flags(pkt, blockflag):
    """-> (long, prev_long, next_long) of one audio packet (4.3.1; bits LSb first)"""
    if not pkt:
        return None
    bits = int.from_bytes(pkt[:4], "little")
    nb = max(0, (len(blockflag) - 1).bit_length())
    mode = (bits >> 1) & ((1 << nb) - 1)
    if mode >= len(blockflag):
        return None
    if not blockflag[mode]:
        return (0, 0, 0)
    return (1, (bits >> (1 + nb)) & 1, (bits >> (2 + nb)) & 1)


def hook_digests(entries, upto):
    """Digests of the reference's hooks of audio packets [0, upto): floor1 ys (with packet and channel), after_residue, and the
    non-PCM hook stream in the form of make_synth_ogg.py. The setup hooks come first."""
    ys, res, hk = hashlib.sha256(), hashlib.sha256(), []
    pk, floor_ch = -1, -1
    for nm, ch, v in entries:
        if nm == "start_audio_packet":
            pk += 1
        if pk >= upto:
            break
        if nm == "floor_number":
            floor_ch = ch
        elif nm == "floor1 ys" and pk >= 0:
            ys.update(np.asarray([pk, floor_ch, len(v)], np.int32).tobytes() + v.astype(np.uint32).tobytes())
        elif nm == "after_residue":
            res.update(np.asarray([pk, ch, len(v)], np.int32).tobytes() + np.ascontiguousarray(v, np.float32).tobytes())
        if nm != "pcm":
            hk.append((nm, ch, v))
    return ys.hexdigest(), res.hexdigest(), hk


def hook_stream(hk):
    """-> (sha256 over names, channels, lengths and integer CRCs, per-hook float sum, per-hook float abs sum (0 for integers))"""
    h = hashlib.sha256()
    sums, abss = [], []
    for nm, ch, v in hk:
        f = v.dtype.kind == "f"
        h.update(("%s|%d|%d|%d|%d;" % (nm, ch, len(v), f, 0 if f else zlib.crc32(v.astype(np.int64).tobytes()))).encode())
        sums.append(float(v.astype(np.float64).sum()) if f else 0.0)
        abss.append(float(np.abs(v.astype(np.float64)).sum()) if f else 0.0)
    return h.hexdigest(), sums, abss


def run_reference(info, data):
    """-> record fields, or (None, why)"""
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "d.ogg")
        open(path, "wb").write(data)
        r = subprocess.run(["timeout", "-k", "10", "120", ASAN, "--in", path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        if b"AddressSanitizer" in r.stdout:
            return None, "memory error"
        if r.returncode not in (0, 1):
            return None, "reference aborted"
        dump = os.path.join(td, "d.bin")
        r = subprocess.run(["timeout", "-k", "10", "120", OURS, "--in", path, "--debug_out", dump], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE)
        if r.returncode not in (0, 1):
            return None, "reference aborted"
        header, entries = read_dump(dump)
    C = int(header["decoder-num-channels"][0])
    pcm = [[] for _ in range(C)]
    started = finished = 0
    blocks = []
    for nm, ch, v in entries:
        if nm == "start_audio_packet":
            started += 1
        elif nm == "finish_audio_packet":
            finished += 1
        elif nm == "pcm":
            pcm[ch].append(np.asarray(v, np.float32))
        elif nm == "pcm_after_mdct" and ch == 0:
            blocks.append(len(v))
    pcm = np.stack([np.concatenate(p) if p else np.zeros(0, np.float32) for p in pcm])
    err = re.sub(r"\S*/(?=[\w.]+:\d+: check failed)", "", r.stderr.decode(errors="replace").strip())  # file names without their directory
    rc = r.returncode
    flag = synthesis_flag(err) if rc else 0
    # the packet the reference failed in (a CHECK inside an audio packet; the granule CHECKs of forwardReadyPcm come after its
    # finish_audio_packet hook), or the one it never started (a page-level error)
    fail_at = -1 if rc == 0 else (started - 1 if started > finished or flag else started)
    # class A from the packets the reference decoded: their block sizes (pcm_after_mdct) and the window flags they carry
    pks = audio_packets(data)
    wf = [window_flags(p, info["blockflag"]) for p in pks[:len(blocks)]]
    assert all(w is not None for w in wf), "packet walk disagrees with the reference"
    bs = sorted(set(blocks))
    assert all((b == max(bs)) == bool(w[0]) or len(bs) == 1 for b, w in zip(blocks, wf)), "block sizes disagree with the modes"
    a_at = -1
    if len(bs) == 2:
        for q in range(len(blocks) - 1):
            if wf[q][0] and wf[q][2] and not wf[q + 1][0]:
                a_at = q + 1
                break
    if a_at >= 0 and (rc == 0 or a_at < fail_at):
        expect = (False, WINDOW_FLAGS, a_at)
    elif rc == 0:
        expect = (True, 0, -1)
    else:
        expect = (False, flag, fail_at)
    upto = expect[2] if expect[2] >= 0 else 1 << 30
    ys, res, hk = hook_digests(entries, upto)
    # PCM the reference delivered in front of the packet where the product stops (class A: the device stops earlier)
    frames = pcm.shape[1]
    if expect[1] == WINDOW_FLAGS:
        frames = sum_frames(entries, a_at)
        pcm = pcm[:, :frames]
    return dict(rc=rc, err=err[-160:], packets=started, frames=frames, pcm=hashlib.sha256(np.ascontiguousarray(pcm).view(np.uint32).tobytes()).hexdigest(),
                ys=ys, res=res, hk=hk, expect=expect, cat=category(rc, flag, expect)), ""


def sum_frames(entries, upto):
    """PCM frames the reference delivered while decoding audio packets [0, upto)"""
    pk, n = -1, 0
    for nm, ch, v in entries:
        if nm == "start_audio_packet":
            pk += 1
            if pk >= upto:
                break
        elif nm == "pcm" and ch == 0:
            n += len(v)
    return n


def category(rc, flag, expect):
    if expect[1] == WINDOW_FLAGS:
        return "class_a"
    if rc == 0:
        return "accepted"
    return "synthesis" if flag else "entropy"


def one(job):
    seed, k, name = job
    info = INFOS[name]
    rng = np.random.default_rng([seed, k])
    kind, edits, trunc = draw(rng, info)
    data = apply(info, edits, trunc)
    if data == info["data"]:
        return job, None, "equals its base"
    rec, why = run_reference(info, data)
    if rec is None:
        return job, None, why
    rec.update(kind=kind, edits=sorted(edits.items()), trunc=trunc, sha=hashlib.sha256(data).hexdigest())
    return job, rec, ""


INFOS = {n: base_info(n) for n in BASES}


def select(cands):
    """The rare records (class A, floor range, floor value: every one the draws produce), then records that meet an open quota, then
    the rest, in draw order, up to TARGET."""
    rare = [c for c in cands if c[1]["expect"][1] in (WINDOW_FLAGS, FLOOR_RANGE, FLOOR_VALUE)]
    chosen = list(rare)
    rest = [c for c in cands if c not in rare]

    def counts(sel):
        cnt = dict(accepted=0, entropy=0, synthesis=0, kind_b=0, kind_d=0)
        per = {n: 0 for n in BASES}
        for (seed, k, name), r in sel:
            cnt[r["cat"]] = cnt.get(r["cat"], 0) + 1
            cnt["kind_" + r["kind"]] = cnt.get("kind_" + r["kind"], 0) + 1
            per[name] += 1
        return cnt, per

    for _ in range(2):
        for c in list(rest):
            cnt, per = counts(chosen)
            (seed, k, name), r = c
            need = (cnt.get(r["cat"], 0) < QUOTA.get(r["cat"], 0) or per[name] < QUOTA["per_base"]
                    or cnt.get("kind_" + r["kind"], 0) < QUOTA.get("kind_" + r["kind"], 0))
            if need:
                chosen.append(c)
                rest.remove(c)
    for c in rest:
        if len(chosen) >= TARGET:
            break
        chosen.append(c)
    chosen.sort(key=lambda c: (BASES.index(c[0][2]), c[0][0], c[0][1]))
    return chosen, counts(chosen)


def main():
    jobs = [(seed, k, BASES[k % len(BASES)]) for seed in SEEDS for k in range(DRAWS_PER_SEED)]
    dropped = {}
    cands = []
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        for job, rec, why in ex.map(one, jobs):
            if rec is None:
                dropped[why] = dropped.get(why, 0) + 1
            else:
                cands.append((job, rec))
    allcnt = {}
    for _, r in cands:
        allcnt[r["cat"]] = allcnt.get(r["cat"], 0) + 1
    print("draws %d: %s; dropped %s" % (len(jobs), allcnt, dropped))
    chosen, (cnt, per) = select(cands)
    print("records %d: %s" % (len(chosen), cnt))
    print("per base: %s" % per)
    assert cnt["accepted"] >= QUOTA["accepted"] and cnt["entropy"] >= QUOTA["entropy"] and cnt["synthesis"] >= QUOTA["synthesis"]
    assert min(per.values()) >= QUOTA["per_base"] and cnt["kind_b"] >= QUOTA["kind_b"] and cnt["kind_d"] >= QUOTA["kind_d"]
    out = dict(base_names=np.asarray(BASES), base=[], seed=[], draw=[], kind=[], trunc=[], sha=[], ref_rc=[], ref_err=[], ref_packets=[],
               ref_frames=[], ref_pcm=[], ref_ys=[], ref_res=[], expect_ok=[], expect_flags=[], expect_bad=[], hook_sha=[], hook_off=[],
               hook_num=[])
    pos, val, eoff, hsum, habs = [], [], [0], [], []
    n_cli_ok = 0
    for (seed, k, name), r in chosen:
        out["base"].append(BASES.index(name))
        out["seed"].append(seed)
        out["draw"].append(k)
        out["kind"].append(r["kind"])
        out["trunc"].append(r["trunc"])
        for p, v in r["edits"]:
            pos.append(p)
            val.append(v)
        eoff.append(len(pos))
        out["sha"].append(r["sha"])
        out["ref_rc"].append(r["rc"])
        out["ref_err"].append(r["err"])
        out["ref_packets"].append(r["packets"])
        out["ref_frames"].append(r["frames"])
        out["ref_pcm"].append(r["pcm"])
        out["ref_ys"].append(r["ys"])
        out["ref_res"].append(r["res"])
        ok, fl, bad = r["expect"]
        out["expect_ok"].append(ok)
        out["expect_flags"].append(fl)
        out["expect_bad"].append(bad)
        cli = not ok or (n_cli_ok < CLI_ACCEPTED and len(out["base"]) % 6 == 0)
        n_cli_ok += ok and cli
        hs, sums, abss = hook_stream(r["hk"])
        out["hook_sha"].append(hs if cli else "")
        out["hook_off"].append(len(hsum))
        out["hook_num"].append(len(sums) if cli else 0)
        if cli:
            hsum += sums
            habs += abss
    arrays = {k: np.asarray(v) for k, v in out.items()}
    for k in ("base", "seed", "draw", "trunc", "ref_rc", "ref_packets", "ref_frames", "expect_bad", "hook_off", "hook_num"):
        arrays[k] = arrays[k].astype(np.int32)
    arrays["expect_flags"] = arrays["expect_flags"].astype(np.uint8)
    arrays.update(edit_pos=np.asarray(pos, np.int32), edit_val=np.asarray(val, np.uint8), edit_off=np.asarray(eoff, np.int32),
                  hook_sum=np.asarray(hsum, np.float64), hook_abs=np.asarray(habs, np.float64))
    path = os.path.join(GOLDEN, "damaged.npz")
    np.savez_compressed(path, **arrays)
    # np.savez_compressed stamps the zip members with the current time: pin them, so that a rerun writes the same bytes
    import zipfile
    tmp = path + ".tmp"
    with zipfile.ZipFile(path) as zin, zipfile.ZipFile(tmp, "w", zipfile.ZIP_DEFLATED) as zout:
        for item in sorted(zin.infolist(), key=lambda i: i.filename):
            zi = zipfile.ZipInfo(item.filename, date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zout.writestr(zi, zin.read(item.filename))
    os.replace(tmp, path)
    print("%s: %d bytes, %d hook digests for the CLI test (%d accepted records)" % (path, os.path.getsize(path), len(hsum),
                                                                                    n_cli_ok))


if __name__ == "__main__":
    main()
