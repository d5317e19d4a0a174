"""PCEN cost. Prints one JSON line per measurement.
--mode kernels: get_spectral_batch(kind="mel_power", n_fft=1024, hop_length=256, n_mels=128, pcen=True, pcen_scale=2**31) on 64
  replicas of test.stereo44khz.ogg in one submit, twice (the first pass warms up). Run it under rocprofv3 --kernel-trace --stats, in
  a run of its own with no counters: the second dispatch of vsyn_pcen_part_kernel, vsyn_pcen_carry_kernel and vsyn_pcen_apply_kernel
  stands beside the second vsyn_spec_stft_kernel, which made the rows they read.
--mode corpus: files/s of the same call with and without pcen=True on a replicated corpus of the two real fixtures, five alternated
  runs each.
Usage: python tools/spectral_pcen_bench.py --mode kernels | corpus [--files 512] [--threads 16] [--feeders 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parseoggvorbis_amd import spectral  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASE = dict(kind="mel_power", n_fft=1024, hop_length=256, n_mels=128)
PCEN = dict(pcen=True, pcen_scale=2 ** 31)


def _ogg(name):
    return open(os.path.join(GOLDEN, name + ".ogg"), "rb").read()


def kernels():
    blobs = [_ogg("test.stereo44khz")] * 64
    for rep in range(2):
        res = spectral.get_spectral_batch(blobs, threads=4, feeders=1, files_per_submit=64, **CASE, **PCEN)
        if rep:
            rows = sum(r.shape[0] for r in res)
            print(json.dumps(dict(measure="kernels", **CASE, **PCEN, rows=rows, blocks_of_64=sum((r.shape[0] + 63) // 64 for r in res),
                                  bytes_written=int(sum(r.nbytes for r in res)))))


def corpus(files, threads, feeders):
    raw = [_ogg("test.stereo44khz"), _ogg("test.mono44khz")]
    blobs = [raw[i % 2] for i in range(files)]
    cases = {"pcen": dict(CASE, **PCEN), "mel_power": CASE}
    times = {k: [] for k in cases}
    for kw in cases.values():
        spectral.get_spectral_batch(blobs, threads=threads, feeders=feeders, **kw)
    for _ in range(5):
        for k, kw in cases.items():
            t0 = time.perf_counter()
            res = spectral.get_spectral_batch(blobs, threads=threads, feeders=feeders, **kw)
            times[k].append(time.perf_counter() - t0)
            del res
    for k, kw in cases.items():
        t = sorted(times[k])
        print(json.dumps(dict(measure="corpus", case=k, **kw, files=files, threads=threads, feeders=feeders,
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
