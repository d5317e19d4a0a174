"""Phase vocoder and PCM stretch cost. Three modes:

  kernels  the workload for one `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/pv_bench.py kernels` run (no
           counters in that run): 64 replicas of tests/golden/test.stereo44khz.ogg's PCM on the device, and per framing (2048 / 512,
           then 1024 / 256) two passes of: the stft rows, the phase vocoder at rate 0.8 on them (block sums, carries, emit), and the
           inverse of the stretched rows (vsyn_istft_frames_kernel + vsyn_istft_ola_kernel). Without the profiler it times the same
           calls, and the whole stage (vsyn_pcm_stretch_device), with device events (second pass).
  report   reads DIR's kernel trace and prints, per framing, each kernel's duration in the SECOND pass, with the bytes it moves and
           the rate, the forward stft kernel and the inverse frame kernel of the same run beside the vocoder's: one JSON line each,
           appended to --out.
  corpus   get_pcm_batch(mono=True) on 64 replicas with and without time_stretch=0.8, alternated --reps times: files/s min / median
           / max, one JSON line each, appended to --out.
Usage: python tools/pv_bench.py kernels | report DIR | corpus [--reps 5] [--out FILE]"""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 64
FRAMINGS = ((2048, 512), (1024, 256))
RATE = 0.8
BLOCK = 64  # VSYN_PV_BLOCK
# what one pass of one framing launches, in order (the offsets kernels and table uploads aside)
PASS = ("vsyn_spec_lin_fft_kernel", "vsyn_pv_kernel", "vsyn_pv_carry_kernel", "vsyn_pv_kernel", "vsyn_istft_frames_kernel", "vsyn_istft_ola_kernel")
ROLE = ("stft", "pv_block_sums", "pv_carries", "pv_emit", "istft_frames", "istft_ola")


def _fixture():
    with open(os.path.join(ROOT, "tests", "golden", "test.stereo44khz.ogg"), "rb") as f:
        return f.read()


def _emit(lines, out):
    with open(out, "a") as f:
        for ln in lines:
            s = json.dumps(ln)
            print(s)
            f.write(s + "\n")


def _shape(T, n, hop):
    F = 1 + T // hop
    return F, int(math.ceil(F / RATE)), int(round(T / RATE)), n // 2 + 1


def kernels(a):
    import numpy as np
    import torch
    from parseoggvorbis_amd import pcm, spectral
    from parseoggvorbis_amd.binding import PcmStretch, Synth
    from tests.workloads import fixture_like_spec
    x, _ = pcm.get_pcm_batch([_fixture()])[0]
    Cn, T = x.shape
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    stream = torch.cuda.current_stream().cuda_stream
    d_pcm = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x, (S, Cn, T)))).cuda()
    d_frames = torch.full((S,), T, dtype=torch.int32, device="cuda")
    lines = []
    for n, hop in FRAMINGS:
        F, Fo, L, nb = _shape(T, n, hop)
        fwd = spectral.spectral_spec("stft", n_fft=n, hop_length=hop)
        st = PcmStretch(n, hop, n, 0, 0, 0)
        d_stft = torch.zeros((S * F, 2 * nb), dtype=torch.float32, device="cuda")
        d_pv = torch.zeros((S * Fo, 2 * nb), dtype=torch.float32, device="cuda")
        d_out = torch.zeros((S, L), dtype=torch.float32, device="cuda")
        steps = (
            ("stft", lambda: g.spectral_device(fwd, [1] * S, d_pcm.data_ptr(), T, Cn, d_frames.data_ptr(), d_stft.data_ptr(), None, stream)),
            ("phase_vocoder", lambda: g.phase_vocoder_device(fwd, [F] * S, [RATE] * S, d_stft.data_ptr(), d_pv.data_ptr(), stream)),
            ("istft", lambda: g.istft_device(fwd, [Fo] * S, d_pv.data_ptr(), None, [L] * S, d_out.data_ptr(), L, None, stream)),
        )
        whole = ("stretch_stage", lambda: g.pcm_stretch_device(st, [T] * S, [RATE] * S, None, d_pcm.data_ptr(), T, Cn, d_out.data_ptr(), L, None, stream))
        for p in range(2):
            for name, fn in steps + ((whole,) if a.stage else ()):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if p == 1:
                    lines.append(dict(measure="events", n_fft=n, hop=hop, step=name, rate=RATE, segments=S, frames=T, rows=S * F, rows_out=S * Fo,
                                      us=round(e0.elapsed_time(e1) * 1e3, 1)))
    g.close()
    _emit(lines, a.out)


def report(a):
    paths = glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(paths) == 1, paths
    with open(paths[0]) as f:
        recs = [r for r in csv.DictReader(f)]
    recs.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"].split("(")[0].split("<")[0].replace(".kd", "").split()[-1] for r in recs]
    mine = [(nm, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for nm, r in zip(names, recs) if nm in set(PASS)]
    per = len(PASS)
    tail = mine[-4 * per:]  # framing 0 pass 0, pass 1, framing 1 pass 0, pass 1: behind the decode's own kernels
    assert len(tail) == 4 * per and [nm for nm, _ in tail] == list(PASS) * 4, [nm for nm, _ in tail]
    from parseoggvorbis_amd import pcm
    x, _ = pcm.get_pcm_batch([_fixture()])[0]
    Cn, T = x.shape
    lines = []
    for i, (n, hop) in enumerate(FRAMINGS):
        F, Fo, L, nb = _shape(T, n, hop)
        rows, rows_out, blocks = S * F, S * Fo, S * ((Fo + BLOCK - 1) // BLOCK)
        pcm_b, in_b, out_b, sum_b, fr_b, y_b = S * Cn * T * 4, rows * nb * 8, rows_out * nb * 8, blocks * nb * 8, rows_out * n * 4, S * L * 4
        # bytes each kernel reads + writes once (a walk reads each input row of its block once, and one more at the block's edge)
        moved = dict(stft=pcm_b + in_b, pv_block_sums=in_b + sum_b, pv_carries=2 * sum_b, pv_emit=in_b + sum_b + out_b, istft_frames=out_b + fr_b,
                     istft_ola=fr_b + y_b)
        second = tail[(2 * i + 1) * per:(2 * i + 2) * per]
        for role, (nm, ns) in zip(ROLE, second):
            lines.append(dict(measure="kernel_trace", n_fft=n, hop=hop, role=role, kernel=nm, rate=RATE, segments=S, frames=T, rows=rows,
                              rows_out=rows_out, us=round(ns / 1e3, 1), mb=round(moved[role] / 1e6, 1), gb_per_s=round(moved[role] / ns, 1),
                              ns_per_bin=round(ns / (rows_out * nb), 4) if role.startswith("pv_") and role != "pv_carries" else None))
    _emit(lines, a.out)


def corpus(a):
    from parseoggvorbis_amd import pcm
    blobs = [_fixture()] * S
    variants = (("mono", dict()), ("mono_time_stretch_0.8", dict(time_stretch=RATE)))
    for _, kw in variants:  # warm-up: library load, workspaces
        pcm.get_pcm_batch(blobs, mono=True, **kw)
    rate = {k: [] for k, _ in variants}
    for _ in range(a.reps):
        for k, kw in variants:
            t0 = time.perf_counter()
            pcm.get_pcm_batch(blobs, mono=True, **kw)
            rate[k].append(S / (time.perf_counter() - t0))
    _emit([dict(measure="corpus_files_per_s", variant=k, files=S, reps=a.reps, min=round(min(v), 1), median=round(statistics.median(v), 1),
                max=round(max(v), 1)) for k, v in rate.items()], a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "report", "corpus"))
    ap.add_argument("dir", nargs="?", default=".")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stage", action="store_true", help="kernels: also time the whole stage (not for a run that report reads)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pv_bench.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    dict(kernels=kernels, report=report, corpus=corpus)[a.mode](a)


if __name__ == "__main__":
    main()
