"""Resampling cost: (1) device time of vsyn_resample_device per hour of 44.1 kHz-length stereo resident on the GPU (16 segments x
225 s at the input rate, HIP events by torch) for 44100->16000, 48000->16000, 16000->44100 and the global-table pair
44056->16000; (2) corpus files/s of get_pcm_batch(sr=16000) against the native float32 run, and of log_mel with sr=16000
against sr=None, on the same replicated corpus of the real fixtures, same threads and feeders. Prints one JSON line per
measurement. Run under rocprofv3 --kernel-trace --stats for the per-kernel split.
Usage: python tools/resample_bench.py [--steps 3] [--files 512] [--threads 16] [--feeders 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from parseoggvorbis_amd import pcm, spectral  # noqa: E402
from parseoggvorbis_amd.binding import Synth  # noqa: E402
from tests.workloads import fixture_like_spec  # noqa: E402

PAIRS = [(44100, 16000), (48000, 16000), (16000, 44100), (44056, 16000)]
GOLDEN = os.path.join(ROOT, "tests", "golden")


def device_per_hour(steps):
    S, Cn, seconds = 16, 2, 225
    dev = torch.device("cuda:0")
    s = Synth(fixture_like_spec(2), device=0, max_streams=4)
    stream = torch.cuda.current_stream(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    for r_in, r_out in PAIRS:
        plane = r_in * seconds
        d_pcm = (torch.rand((S, Cn, plane), generator=gen, device=dev) - 0.5) * 0.5
        d_frames = torch.full((S,), plane, dtype=torch.int32, device=dev)
        out_plane = s.lib.vsyn_resample_num_frames(r_in, r_out, plane)
        d_out = torch.empty((S, Cn, out_plane), dtype=torch.float32, device=dev)
        d_of = torch.empty((S,), dtype=torch.int32, device=dev)
        run = lambda: s.resample_device([r_in] * S, r_out, d_pcm.data_ptr(), plane, Cn, d_frames.data_ptr(), d_out.data_ptr(),  # noqa: E731
                                        out_plane, d_of.data_ptr(), stream.cuda_stream)
        run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(steps):
            run()
        e1.record(stream)
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / steps
        hours = S * seconds / 3600.0
        gb = (S * Cn * plane + S * Cn * out_plane) * 4 / 1e9
        print(json.dumps(dict(measure="device_per_hour", r_in=r_in, r_out=r_out, outputs=S * Cn * out_plane, audio_hours=hours,
                              device_ms=round(ms, 3), ms_per_audio_hour=round(ms / hours, 3), pcm_gb_per_s=round(gb / (ms / 1e3), 1))))
        del d_pcm, d_out
    s.close()


def corpus(files, threads, feeders, steps):
    names = ["test.stereo44khz", "test.mono44khz"]
    raw = [open(os.path.join(GOLDEN, n + ".ogg"), "rb").read() for n in names]
    blobs = [raw[i % 2] for i in range(files)]
    kw = dict(kind="log_mel", n_fft=400, hop_length=160, n_mels=80)
    runs = [("pcm_f32", lambda: pcm.get_pcm_batch(blobs, threads=threads, feeders=feeders)),
            ("pcm_f32_sr16000", lambda: pcm.get_pcm_batch(blobs, sr=16000, threads=threads, feeders=feeders)),
            ("log_mel", lambda: spectral.get_spectral_batch(blobs, threads=threads, feeders=feeders, **kw)),
            ("log_mel_sr16000", lambda: spectral.get_spectral_batch(blobs, sr=16000, threads=threads, feeders=feeders, **kw))]
    for label, run in runs:
        run()
        best = None
        for _ in range(steps):
            t0 = time.perf_counter()
            run()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        print(json.dumps(dict(measure="corpus", run=label, files=files, threads=threads, feeders=feeders, best_s=round(best, 4),
                              files_per_s=round(files / best, 1))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--feeders", type=int, default=3)
    a = ap.parse_args()
    device_per_hour(a.steps)
    corpus(a.files, a.threads, a.feeders, a.steps)


if __name__ == "__main__":
    main()
