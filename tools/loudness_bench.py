"""Loudness cost. Prints one JSON line per measurement.
--mode kernels: get_loudness_batch on 64 replicas of test.stereo44khz.ogg in one submit, then get_pcm_batch(mono=True,
  loudness_normalize=-23) on the same files, each twice (the first pass warms up). Run it under rocprofv3 --kernel-trace --stats, in a
  run of its own with no counters: the dispatches of vsyn_loud_part_kernel, vsyn_loud_carry_kernel, vsyn_loud_apply_kernel,
  vsyn_loud_hops_kernel, vsyn_loud_gate_kernel and vsyn_loud_scale_kernel stand beside the synthesis kernels of the same files.
--mode corpus: files/s of get_loudness_batch, of get_pcm_batch(mono=True) with and without loudness_normalize=-23, and of
  get_spectral_batch(log_mel) with and without it, on a replicated corpus of the two real fixtures, five alternated runs each.
Usage: python tools/loudness_bench.py --mode kernels | corpus [--files 512] [--threads 16] [--feeders 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parseoggvorbis_amd import loudness, pcm, spectral  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MEL = dict(kind="log_mel", n_fft=1024, hop_length=256, n_mels=128)


def _ogg(name):
    return open(os.path.join(GOLDEN, name + ".ogg"), "rb").read()


def kernels():
    blobs = [_ogg("test.stereo44khz")] * 64
    for rep in range(2):
        res = loudness.get_loudness_batch(blobs, threads=4, feeders=1, files_per_submit=64, blocks=True)
        got = pcm.get_pcm_batch(blobs, threads=4, feeders=1, files_per_submit=64, mono=True, loudness_normalize=-23.0)
        if rep:
            print(json.dumps(dict(measure="kernels", files=len(blobs), lufs=round(res[0][0], 4), sr=res[0][1], blocks=int(len(res[0][2])),
                                  frames=int(got[0][0].shape[0]), tiles_of_8192=int(-(-got[0][0].shape[0] // 8192)))))


def corpus(files, threads, feeders):
    raw = [_ogg("test.stereo44khz"), _ogg("test.mono44khz")]
    blobs = [raw[i % 2] for i in range(files)]
    kw = dict(threads=threads, feeders=feeders)
    cases = {
        "loudness": lambda: loudness.get_loudness_batch(blobs, **kw),
        "pcm_mono": lambda: pcm.get_pcm_batch(blobs, mono=True, **kw),
        "pcm_mono_normalized": lambda: pcm.get_pcm_batch(blobs, mono=True, loudness_normalize=-23.0, **kw),
        "log_mel": lambda: spectral.get_spectral_batch(blobs, **MEL, **kw),
        "log_mel_normalized": lambda: spectral.get_spectral_batch(blobs, loudness_normalize=-23.0, **MEL, **kw),
    }
    times = {k: [] for k in cases}
    for fn in cases.values():
        fn()
    for _ in range(5):
        for k, fn in cases.items():
            t0 = time.perf_counter()
            res = fn()
            times[k].append(time.perf_counter() - t0)
            del res
    for k in cases:
        t = sorted(times[k])
        print(json.dumps(dict(measure="corpus", case=k, files=files, threads=threads, feeders=feeders,
                              files_per_s=[round(files / x, 1) for x in (t[-1], t[2], t[0])], note="min / median / max of 5")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernels", "corpus"), required=True)
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--feeders", type=int, default=3)
    a = ap.parse_args()
    if a.mode == "kernels":
        kernels()
    else:
        corpus(a.files, a.threads, a.feeders)


if __name__ == "__main__":
    main()
