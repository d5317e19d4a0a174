"""Linear-spectra cost. Prints one JSON line per measurement.
--mode kernels: get_spectral_batch on 64 replicas of test.stereo44khz.ogg (one submit), once per case, in a fixed order and twice
  over (the first pass warms up): lin_power 2048/512, mel_power 2048/512, lin_power 512/160, mel_power 512/160, stft 1024/256,
  mel_power 1024/256. Run it under rocprofv3 --kernel-trace --stats: the n-th dispatch of vsyn_spec_lin_fft_kernel and of
  vsyn_spec_stft_kernel in the trace belong to the n-th linear resp. mel case. Prints each case's rows and bytes written.
--mode corpus: files/s of get_spectral_batch(kind="lin_power") beside kind="log_mel" at 1024/256 on a replicated corpus of the two
  real fixtures, five alternated runs each.
Usage: python tools/spectral_lin_bench.py --mode kernels | corpus [--files 512] [--threads 16] [--feeders 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parseoggvorbis_amd import spectral  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
KERNEL_CASES = [dict(kind="lin_power", n_fft=2048, hop_length=512), dict(kind="mel_power", n_fft=2048, hop_length=512),
                dict(kind="lin_power", n_fft=512, hop_length=160), dict(kind="mel_power", n_fft=512, hop_length=160),
                dict(kind="stft", n_fft=1024, hop_length=256), dict(kind="mel_power", n_fft=1024, hop_length=256)]


def _ogg(name):
    return open(os.path.join(GOLDEN, name + ".ogg"), "rb").read()


def kernels():
    blobs = [_ogg("test.stereo44khz")] * 64
    for rep in range(2):
        for kw in KERNEL_CASES:
            res = spectral.get_spectral_batch(blobs, threads=4, feeders=1, files_per_submit=64, **kw)
            if rep:
                rows = sum(r.shape[0] for r in res)
                print(json.dumps(dict(measure="kernels", **kw, rows=rows, bytes_written=int(sum(r.nbytes for r in res)))))


def corpus(files, threads, feeders):
    raw = [_ogg("test.stereo44khz"), _ogg("test.mono44khz")]
    blobs = [raw[i % 2] for i in range(files)]
    cases = [dict(kind="lin_power", n_fft=1024, hop_length=256), dict(kind="log_mel", n_fft=1024, hop_length=256)]
    times = {kw["kind"]: [] for kw in cases}
    nbytes = {}
    for kw in cases:
        spectral.get_spectral_batch(blobs, threads=threads, feeders=feeders, **kw)
    for _ in range(5):
        for kw in cases:
            t0 = time.perf_counter()
            res = spectral.get_spectral_batch(blobs, threads=threads, feeders=feeders, **kw)
            times[kw["kind"]].append(time.perf_counter() - t0)
            nbytes[kw["kind"]] = int(sum(r.nbytes for r in res))
            del res
    for kw in cases:
        t = sorted(times[kw["kind"]])
        print(json.dumps(dict(measure="corpus", **kw, files=files, threads=threads, feeders=feeders,
                              files_per_s=[round(files / x, 1) for x in (t[-1], t[2], t[0])], note="min / median / max of 5",
                              bytes_returned=nbytes[kw["kind"]])))


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
