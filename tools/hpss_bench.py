"""HPSS cost. Times, with device events in one process, the spectral kernel that makes a batch's rows and the HPSS
stage alone on those rows: 64 segments of 4 s of noise at 44.1 kHz, n_fft 2048, hop 512 (345 rows each), as "lin_power" rows (1025
bins) and as "mel_power" rows (128 mels); the stage at kernel sizes 31 / 31 and 63 / 63 for the harmonic component (power 2), the
harmonic mask and the time median alone. Every figure is the mean of --reps calls behind --warmup calls, in microseconds. One JSON
line per measurement, printed and appended to --out (default profiles/hpss_bench.txt).
--tree DIR imports parseoggvorbis_amd from another checkout (built there): on a commit without the stage only the spectral kernels
are timed, which is how the parent commit's lin_power time for the same batch is taken; --label names the lines.
Usage: python tools/hpss_bench.py [--tree DIR] [--label NAME] [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, SECONDS, RATE, N_FFT, HOP = 64, 4, 44100, 2048, 512
KINDS = (dict(kind="lin_power", n_fft=N_FFT, hop_length=HOP), dict(kind="mel_power", n_fft=N_FFT, hop_length=HOP, n_mels=128))
STAGES = (dict(), dict(output="mask"), dict(output="median"))


def _timed(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpss_bench.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(1, ROOT)  # tests.workloads
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "hpss_bench needs a GPU"
    from parseoggvorbis_amd import spectral
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    stream = torch.cuda.current_stream().cuda_stream
    plane = SECONDS * RATE
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_pcm = torch.randn((S, 1, plane), generator=gen, device="cuda", dtype=torch.float32) * 0.1
    d_frames = torch.full((S,), plane, dtype=torch.int32, device="cuda")
    d_off = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    has_stage = hasattr(g, "spectral_hpss_device")
    lines = []
    for kw in KINDS:
        spec = spectral.spectral_spec(**kw)
        dim = spectral.spec_dim(spec)
        F = 1 + plane // HOP
        d_rows = torch.zeros((S * F, dim), dtype=torch.float32, device="cuda")
        d_out = torch.zeros_like(d_rows)
        t = _timed(lambda: g.spectral_device(spec, [RATE] * S, d_pcm.data_ptr(), plane, 1, d_frames.data_ptr(), d_rows.data_ptr(),
                                             d_off.data_ptr(), stream), a.warmup, a.reps)
        off = d_off.cpu().numpy()
        assert list(np.diff(off)) == [F] * S, off
        mb = S * F * dim * 4 / 1e6
        lines.append(dict(measure="spectral", label=a.label, kind=kw["kind"], segments=S, rows=S * F, dim=dim, us=round(t, 1), rows_mb=round(mb, 1)))
        if not has_stage:
            continue
        for k in (31, 63):
            for st in STAGES:
                hp = spectral.hpss_spec("harmonic", k, 2.0, 1.0, st.get("output", "component"))
                t = _timed(lambda: g.spectral_hpss_device(hp, dim, [F] * S, d_rows.data_ptr(), d_out.data_ptr(), stream), a.warmup, a.reps)
                lines.append(dict(measure="hpss", label=a.label, kind=kw["kind"], kernel=[k, k], output=st.get("output", "component"), rows=S * F,
                                  dim=dim, us=round(t, 1), gb_per_s=round(2 * mb / t * 1e3, 1), note="gb_per_s: rows read once + written once"))
        tp = _timed(lambda: g.spectral_hpss_device(hp, dim, [F] * S, d_rows.data_ptr(), d_rows.data_ptr(), stream), a.warmup, a.reps)
        lines.append(dict(measure="hpss_in_place", label=a.label, kind=kw["kind"], kernel=[63, 63], output="median", us=round(tp, 1)))
    g.close()
    with open(a.out, "a") as f:
        for ln in lines:
            s = json.dumps(ln)
            print(s)
            f.write(s + "\n")


if __name__ == "__main__":
    main()
