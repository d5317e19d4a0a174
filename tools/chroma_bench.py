"""Chroma cost against the linear spectrum it is built from: device-side time of one call of vsyn_spectral_chroma_device
(kinds chroma and tonnetz) and of vsyn_spectral_device (lin_power) on the same resident PCM, 64 segments x 10 s of 44.1 kHz mono, at
n_fft 2048 / hop 512 (FFT path) and n_fft 1102 / hop 441 (direct path). The calls of a case are alternated with the other cases' in
every round; per case the median over the rounds of HIP-event time around one call (table upload, offsets kernel, the kernel).
Prints one JSON line per case. Run under rocprofv3 --kernel-trace --stats for the kernels alone.
--root DIR imports the package from another checkout (the parent commit, say) to time its lin_power in the same process layout; a
checkout without the chroma kinds times lin_power alone (--kinds lin_power does the same here, for a like-for-like comparison: what
else runs between two calls moves the clocks).
Usage: python tools/chroma_bench.py [--rounds 20] [--root DIR] [--kinds lin_power,chroma,tonnetz]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--kinds", default="lin_power,chroma,tonnetz")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from parseoggvorbis_amd import spectral
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec

    S, sr, seconds = 64, 44100, 10
    plane = sr * seconds
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    d_pcm = (torch.rand((S, 1, plane), generator=gen, device=dev) - 0.5) * 0.5
    d_frames = torch.full((S,), plane, dtype=torch.int32, device=dev)
    d_off = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    s = Synth(fixture_like_spec(2), device=0, max_streams=4)
    stream = torch.cuda.current_stream(dev)
    chroma_kinds = getattr(spectral, "CHROMA_KINDS", {})  # (a checkout without them)
    kinds = [k for k in a.kinds.split(",") if k in spectral.KINDS or k in chroma_kinds]
    cases = []
    for n_fft, hop in ((2048, 512), (1102, 441)):
        for kind in kinds:
            sp = spectral.spectral_spec(kind, n_fft=n_fft, hop_length=hop)
            F = s.lib.vsyn_spectral_num_frames(C.byref(sp), plane)
            dim = spectral.spec_dim(sp, spectral.chroma_spec()) if kind in chroma_kinds else spectral.spec_dim(sp)
            d_rows = torch.empty((S * F, dim), dtype=torch.float32, device=dev)
            run = (lambda sp=sp, d_rows=d_rows: s.spectral_device(sp, [sr] * S, d_pcm.data_ptr(), plane, 1, d_frames.data_ptr(), d_rows.data_ptr(),
                                                                   d_off.data_ptr(), stream.cuda_stream))
            cases.append((dict(kind=kind, n_fft=n_fft, hop_length=hop, rows=S * F, dim=int(d_rows.shape[1])), run, []))
    for _, run, _ in cases:  # warm-up: code objects, workspaces
        run()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for _, run, ms in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run()
            e1.record(stream)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
    for info, _, ms in cases:
        print(json.dumps(dict(measure="chroma_bench", root=os.path.abspath(a.root), **info, rounds=a.rounds, median_ms=round(statistics.median(ms), 4),
                              min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))))
    s.close()


if __name__ == "__main__":
    main()
