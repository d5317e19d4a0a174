"""Spectral-feature cost: (1) device time of vsyn_spectral_device per hour of 44.1 kHz stereo audio resident on the GPU (16
segments x 225 s, HIP events by torch) for 1102/441/80 log_mel and 2048/512/128 mfcc; (2) ogg_vorbis_spectral_corpus files/s
against ogg_vorbis_decode_corpus (float32 PCM copied back) on the same replicated corpus of the real fixtures, same threads and
feeders. Prints one JSON line per measurement. Run under rocprofv3 --kernel-trace --stats for the per-kernel split.
Usage: python tools/spectral_bench.py [--steps 3] [--files 512] [--threads 16] [--feeders 3]"""
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

CASES = [dict(kind="log_mel", n_fft=1102, hop_length=441, n_mels=80), dict(kind="mfcc", n_fft=2048, hop_length=512, n_mels=128)]
GOLDEN = os.path.join(ROOT, "tests", "golden")


def device_per_hour(steps):
    S, Cn, sr, seconds = 16, 2, 44100, 225
    plane = sr * seconds
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    d_pcm = (torch.rand((S, Cn, plane), generator=g, device=dev) - 0.5) * 0.5
    d_frames = torch.full((S,), plane, dtype=torch.int32, device=dev)
    d_off = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    s = Synth(fixture_like_spec(2), device=0, max_streams=4)
    stream = torch.cuda.current_stream(dev)
    for kw in CASES:
        sp = spectral.spectral_spec(**kw)
        F = s.lib.vsyn_spectral_num_frames(C.byref(sp), plane)
        d_rows = torch.empty((S * F, spectral.spec_dim(sp)), dtype=torch.float32, device=dev)
        run = lambda: s.spectral_device(sp, [sr] * S, d_pcm.data_ptr(), plane, Cn, d_frames.data_ptr(), d_rows.data_ptr(), d_off.data_ptr(),  # noqa: E731
                                        stream.cuda_stream)
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
        print(json.dumps(dict(measure="device_per_hour", **kw, rows=S * F, audio_hours=hours, device_ms=round(ms, 2),
                              ms_per_audio_hour=round(ms / hours, 2), realtime_factor=round(hours * 3600e3 / ms))))
    s.close()


def corpus(files, threads, feeders, steps):
    lib = spectral._load()
    lib.ogg_vorbis_decode_corpus.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_int,
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_char_p)]
    lib.ogg_vorbis_decode_corpus.restype = C.c_int
    names = ["test.stereo44khz", "test.mono44khz"]
    raw = [open(os.path.join(GOLDEN, n + ".ogg"), "rb").read() for n in names]
    blobs = [raw[i % 2] for i in range(files)]
    n, cap = len(blobs), 131072
    chans = [b[27 + b[26] + 11] for b in blobs]
    datas = (C.c_char_p * n)(*blobs)
    lens = (C.c_size_t * n)(*[len(b) for b in blobs])
    pcm = [np.zeros((chans[i], cap), np.float32) for i in range(n)]
    ptrs = (C.c_void_p * n)(*[p.ctypes.data for p in pcm])
    caps = (C.c_uint64 * n)(*([cap] * n))
    frames, sums, ok = (C.c_uint64 * n)(), (C.c_double * n)(), (C.c_uint8 * n)()
    err = C.c_char_p()

    def pcm_run():
        assert lib.ogg_vorbis_decode_corpus(datas, lens, n, threads, feeders, 64, 0, frames, sums, ok, ptrs, caps, None, C.byref(err)) == 0
        assert all(ok)

    audio_s = None
    for label, run in [("pcm_f32", pcm_run)] + [("spectral_" + kw["kind"], (lambda kw=kw: spectral.get_spectral_batch(
            blobs, threads=threads, feeders=feeders, **kw))) for kw in CASES]:
        run()
        best = None
        for _ in range(steps):
            t0 = time.perf_counter()
            run()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        if audio_s is None:
            audio_s = sum(frames[i] for i in range(n)) / 44100.0
        print(json.dumps(dict(measure="corpus", run=label, files=n, threads=threads, feeders=feeders, best_s=round(best, 4),
                              files_per_s=round(n / best, 1), audio_x_realtime=round(audio_s / best))))


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
