"""Rhythm cost. Times each device form alone, with device events in one process, next to the mel_db kernel that makes
the rows: 64 segments of 91136 samples of noise at 44.1 kHz (the shape of DESIGN.md 6i), n_fft 2048, hop 512, 128 mels: 179 rows a
segment. Measured: the mel_db kernel and, for the comparison with the parent commit, the lin_power kernel of the same batch; the
onset stage at (lag, max_size) = (1, 1) and (2, 3); the peak picker with librosa's times; the tempogram at win_length 384 as rows, as
rows + mean and as the mean alone, and the mean alone at 689 (tempo's window at this rate).
Every measurement is --reps calls behind --warmup calls, each call between its own pair of events: min / median / max in
microseconds, and for the tempogram the float64 fma rate that is. One JSON line per measurement, printed and appended to --out
(default profiles/rhythm_bench.txt).
--tree DIR imports parseoggvorbis_amd from another checkout (built there): on a commit without the stages only the spectral kernel
is timed, which is how the parent commit's time for the same batch is taken; --label names the lines.
Usage: python tools/rhythm_bench.py [--tree DIR] [--label NAME] [--reps 10] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, SAMPLES, RATE, N_FFT, HOP, N_MELS = 64, 91136, 44100, 2048, 512, 128


def _timed(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0)
    ts.sort()
    return dict(us_min=round(ts[0], 1), us_median=round(ts[len(ts) // 2], 1), us_max=round(ts[-1], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rhythm_bench.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(1, ROOT)  # tests.workloads
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "rhythm_bench needs a GPU"
    from parseoggvorbis_amd import binding, spectral
    from tests.workloads import fixture_like_spec
    g = binding.Synth(fixture_like_spec(2), device=0, max_streams=4)
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_pcm = torch.randn((S, 1, SAMPLES), generator=gen, device="cuda", dtype=torch.float32) * 0.1
    d_frames = torch.full((S,), SAMPLES, dtype=torch.int32, device="cuda")
    d_off = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    spec = spectral.spectral_spec(kind="mel_db", n_fft=N_FFT, hop_length=HOP, n_mels=N_MELS)
    F = 1 + SAMPLES // HOP
    d_rows = torch.zeros((S * F, N_MELS), dtype=torch.float32, device="cuda")
    base = dict(label=a.label, segments=S, rows=S * F)
    lines = [dict(measure="spectral", kind="mel_db", dim=N_MELS, **base,
                  **_timed(lambda: g.spectral_device(spec, [RATE] * S, d_pcm.data_ptr(), SAMPLES, 1, d_frames.data_ptr(), d_rows.data_ptr(),
                                                     d_off.data_ptr(), stream), a.warmup, a.reps))]
    assert list(np.diff(d_off.cpu().numpy())) == [F] * S
    lin = spectral.spectral_spec(kind="lin_power", n_fft=N_FFT, hop_length=HOP)
    d_lin = torch.zeros((S * F, N_FFT // 2 + 1), dtype=torch.float32, device="cuda")
    lines.append(dict(measure="spectral", kind="lin_power", dim=N_FFT // 2 + 1, **base,
                      **_timed(lambda: g.spectral_device(lin, [RATE] * S, d_pcm.data_ptr(), SAMPLES, 1, d_frames.data_ptr(), d_lin.data_ptr(),
                                                         d_off.data_ptr(), stream), a.warmup, a.reps)))
    del d_lin
    if hasattr(g, "onset_strength_device"):
        rows, rates = [F] * S, [RATE] * S
        d_env = torch.zeros(S * F, dtype=torch.float32, device="cuda")
        for lag, m in ((1, 1), (2, 3)):
            on = binding.OnsetSpec(lag, m, N_FFT, HOP, 1)
            lines.append(dict(measure="onset_strength", lag=lag, max_size=m, dim=N_MELS, **base,
                              **_timed(lambda: g.onset_strength_device(on, N_MELS, rows, d_rows.data_ptr(), d_env.data_ptr(), stream), a.warmup, a.reps)))
        pk = binding.OnsetPeaks(0.03, 0.0, 0.10, 0.10, 0.03, 0.07, HOP, 1)
        d_on = torch.zeros(S * F, dtype=torch.int32, device="cuda")
        d_cnt = torch.zeros(S, dtype=torch.int32, device="cuda")
        lines.append(dict(measure="onset_peaks", windows=list(binding.onset_peak_windows(pk, RATE)), **base,
                          **_timed(lambda: g.onset_peaks_device(pk, rows, rates, d_env.data_ptr(), d_on.data_ptr(), d_cnt.data_ptr(), None, stream),
                                   a.warmup, a.reps)))
        lines[-1]["onsets"] = int(d_cnt.sum().item())
        for W, want_rows, want_mean in ((384, True, False), (384, True, True), (384, False, True), (689, False, True)):
            tg = binding.TempogramSpec(W, HOP, 3, 0, 0.0)
            d_tg = torch.zeros(S * F * W if want_rows else 1, dtype=torch.float32, device="cuda")
            d_mean = torch.zeros(S * W, dtype=torch.float64, device="cuda")
            t = _timed(lambda: g.tempogram_device(tg, rows, None, d_env.data_ptr(), d_tg.data_ptr() if want_rows else None,
                                                  d_mean.data_ptr() if want_mean else None, stream), a.warmup, a.reps)
            fma = S * F * W * (W + 1) // 2
            lines.append(dict(measure="tempogram", win_length=W, out=("rows" if want_rows else "") + ("+mean" if want_rows and want_mean else "mean" if want_mean else ""),
                              tile=g.lib.vsyn_tempogram_tile(W), fma=fma, gfma_per_s=round(fma / t["us_median"] / 1e3, 1), **base, **t))
    g.close()
    with open(a.out, "a") as f:
        for ln in lines:
            s = json.dumps(ln)
            print(s)
            f.write(s + "\n")


if __name__ == "__main__":
    main()
