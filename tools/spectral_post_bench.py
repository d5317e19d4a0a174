"""Cost of the spectral post stage (delta=2, mean_var) for log_mel 1102/441/80, beside tools/spectral_bench.py:
(1) device time per hour of 44.1 kHz stereo audio resident on the GPU (16 segments x 225 s, HIP events by torch) of
vsyn_spectral_device alone and followed by vsyn_spectral_post_device, alternated in one process; the first call of each (code object
load, workspace growth) is reported apart from the warm ones; (2) get_spectral_batch files/s over a replicated corpus of the real
fixtures with the stage off and on, alternated, `--repeats` each: the spread of the "off" runs is the noise the "on" runs are read
against; two more variants separate the stage from the width of its rows (normalisation alone: 80 columns; the stage off with
n_mels=240: as many columns as the "on" run delivers); (3) the bytes each of the stage's kernels must move for (1), to set against
the kernel times of a rocprofv3 --kernel-trace --stats run of this script (--only device). Prints one JSON line per measurement.
Usage: python tools/spectral_post_bench.py [--steps 5] [--repeats 3] [--files 512] [--threads 16] [--feeders 3] [--only device|corpus]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from parseoggvorbis_amd import spectral  # noqa: E402
from parseoggvorbis_amd.binding import Synth  # noqa: E402
from tests.workloads import fixture_like_spec  # noqa: E402

CASE = dict(kind="log_mel", n_fft=1102, hop_length=441, n_mels=80)
POST = dict(delta=2, delta_width=9, normalize="mean_var")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def device_per_hour(steps):
    S, Cn, sr, seconds = 16, 2, 44100, 225
    plane = sr * seconds
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    d_pcm = (torch.rand((S, Cn, plane), generator=gen, device=dev) - 0.5) * 0.5
    d_frames = torch.full((S,), plane, dtype=torch.int32, device=dev)
    d_off = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    s = Synth(fixture_like_spec(2), device=0, max_streams=4)
    stream = torch.cuda.current_stream(dev)
    sp = spectral.spectral_spec(**CASE)
    post, dout, _ = spectral.post_spec(spectral.spec_dim(sp), **POST)
    D = spectral.spec_dim(sp)
    F = s.lib.vsyn_spectral_num_frames(C.byref(sp), plane)
    d_rows = torch.empty((S * F, D), dtype=torch.float32, device=dev)
    d_out = torch.empty((S * F, dout), dtype=torch.float32, device=dev)

    def spec_only():
        s.spectral_device(sp, [sr] * S, d_pcm.data_ptr(), plane, Cn, d_frames.data_ptr(), d_rows.data_ptr(), d_off.data_ptr(), stream.cuda_stream)

    def post_only():
        s.spectral_post_device(post, D, [F] * S, d_rows.data_ptr(), d_out.data_ptr(), stream.cuda_stream)

    def both():
        spec_only()
        post_only()

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    hours = S * seconds / 3600.0
    first = {name: timed(fn, 1) for name, fn in (("spectral", spec_only), ("post", post_only))}
    warm = {"spectral": [], "spectral+post": [], "post": []}
    for _ in range(3):  # alternated
        warm["spectral"].append(timed(spec_only, steps))
        warm["spectral+post"].append(timed(both, steps))
        warm["post"].append(timed(post_only, 10 * steps))
    for name, ms in warm.items():
        print(json.dumps(dict(measure="device_per_hour", run=name, **CASE, **(POST if "post" in name else {}), rows=S * F, audio_hours=hours,
                              first_call_ms=round(first[name], 3) if name in first else None, warm_ms=[round(m, 3) for m in ms],
                              ms_per_audio_hour=round(min(ms) / hours, 3))))
    # what the stage's kernels must move, for the per-kernel times of a kernel trace
    n = S * F
    for kernel, nbytes in (("vsyn_post_delta_kernel", 4 * n * (D + dout)), ("vsyn_post_moment_kernel", 4 * n * dout),
                           ("vsyn_post_norm_kernel", 8 * n * dout), ("vsyn_post_reduce_kernel", 8 * ((F + 15) // 16) * S * dout)):
        print(json.dumps(dict(measure="kernel_bytes", kernel=kernel, rows=n, dim=D, dim_out=dout, bytes=nbytes)))
    s.close()


def corpus(files, threads, feeders, repeats):
    names = ["test.stereo44khz", "test.mono44khz"]
    raw = [open(os.path.join(GOLDEN, n + ".ogg"), "rb").read() for n in names]
    blobs = [raw[i % 2] for i in range(files)]
    # "norm_only" keeps the rows 80 wide (the stage's launches and workspace alone); "off_240" is the stage off with n_mels = 240:
    # rows as wide as the "on" run's, i.e. what delivering 240 columns per frame to the host costs without the stage
    variants = {"off": {}, "norm_only": dict(normalize="mean_var"), "on": POST, "off_240": dict(n_mels=240)}
    runs = {k: (lambda kw=kw: spectral.get_spectral_batch(blobs, threads=threads, feeders=feeders, **{**CASE, **kw})) for k, kw in variants.items()}
    for fn in runs.values():
        fn()
    times = {k: [] for k in runs}
    for _ in range(repeats):  # alternated
        for label, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            times[label].append(time.perf_counter() - t0)
    for label, ts in times.items():
        print(json.dumps(dict(measure="corpus", post=label, **{**CASE, **variants[label]}, files=files, threads=threads, feeders=feeders,
                              seconds=[round(t, 4) for t in ts], files_per_s=[round(files / t, 1) for t in ts])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--feeders", type=int, default=3)
    ap.add_argument("--only", choices=["device", "corpus"])
    a = ap.parse_args()
    if a.only != "corpus":
        device_per_hour(a.steps)
    if a.only != "device":
        corpus(a.files, a.threads, a.feeders, a.repeats)


if __name__ == "__main__":
    main()
