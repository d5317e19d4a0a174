"""The constant-Q stage timed with device events (profiles/cqt_bench.txt): 64 mono segments of 10 s at 22 050 Hz,
hop_length 512, at librosa.cqt's defaults (84 bins, 12 per octave) and at chroma_cqt's (252 bins, 36 per octave, folded to 12 chroma),
beside the yardstick: the direct-DFT chroma kernel at n_fft = 1102 on the same PCM in the same process. Three warm-up rounds and ten
timed ones per case, alternated; prints the medians, the complex-MAC rates (F * sum_k L_k per segment for the constant-Q cases,
F * NB * n_fft for the direct DFT) and the bytes of wavelet table a frame tile reads. Run from the repository root with PYTHONPATH
set to it; under rocprofv3 --kernel-trace --stats -- python profiles/cqt_bench.py for the kernels' own times. Does not touch
bench.py."""
import ctypes as C

import numpy as np
import torch

from parseoggvorbis_amd import binding, cqt, spectral
from parseoggvorbis_amd.binding import Synth
from tests.workloads import fixture_like_spec

S, T, SR, HOP = 64, 220500, 22050, 512
handles = [Synth(fixture_like_spec(2), device=0, max_streams=4) for _ in range(3)]  # one per case: a handle keeps one wavelet table
rng = np.random.default_rng(5)
t = np.arange(T) / SR
x = np.stack([sum(0.2 * np.cos(2 * np.pi * f * t + p) for f, p in zip(rng.uniform(60, 4000, 4), rng.uniform(0, 6, 4))) + 0.05 * rng.standard_normal(T)
              for _ in range(S)]).astype(np.float32)
d_pcm = torch.from_numpy(x).cuda()
d_frames = torch.full((S,), T, dtype=torch.int32, device="cuda")
F = 1 + T // HOP
d_rows = torch.zeros((S * F + 8) * 252, dtype=torch.float32, device="cuda")
d_ref = torch.zeros(S, dtype=torch.int32, device="cuda")
st = torch.cuda.current_stream().cuda_stream
rates = [SR] * S

cases = []
for g, (name, sp) in zip(handles, (("cqt 84 bins / 12 per octave, magnitude", cqt.cqt_spec(hop_length=HOP)),
                 ("chroma_cqt 252 bins / 36 per octave", cqt.cqt_spec(hop_length=HOP, n_bins=252, bins_per_octave=36, output="chroma")))):
    rc, N, L = binding.cqt_lengths(sp, SR)
    assert rc == 0
    total = int(L.astype(np.int64).sum())
    ft, chunk, bpw = binding.cqt_tile(sp, SR)
    cases.append((name, lambda sp=sp, g=g: g.cqt_device(sp, rates, d_pcm.data_ptr(), T, 1, d_frames.data_ptr(), d_rows.data_ptr(), None, d_ref.data_ptr(), st),
                  F * total, "L_0 %d, sum L %d, tile %d frames x %d bins, chunk %d, table read per frame tile %.2f MB" % (L[0], total, ft, bpw, chunk, 8e-6 * total)))
ch = spectral.spectral_spec(kind="chroma", n_fft=1102, hop_length=HOP)
g = handles[2]
Fc = int(g.lib.vsyn_spectral_num_frames(C.byref(ch), T))
cases.append(("yardstick: chroma_stft, direct DFT n_fft 1102",
              lambda: g.spectral_chroma_device(ch, None, rates, d_pcm.data_ptr(), T, 1, d_frames.data_ptr(), d_rows.data_ptr(), None, st),
              Fc * 552 * 1102, "NB 552, %d frames" % Fc))

ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in cases]
times = [[] for _ in cases]
for it in range(13):
    for i, (_, run, _, _) in enumerate(cases):
        ev[i][0].record()
        run()
        ev[i][1].record()
    torch.cuda.synchronize()
    if it >= 3:
        for i in range(len(cases)):
            times[i].append(ev[i][0].elapsed_time(ev[i][1]))
assert not d_ref.cpu().numpy().any()
for (name, _, macs, note), tm in zip(cases, times):
    med = float(np.median(tm))
    print("%s: median of 10 %.3f ms (min %.3f, max %.3f) for %d segments; %.3g complex MAC per segment, %.2f T complex MAC/s; %s"
          % (name, med, min(tm), max(tm), S, macs, S * macs / (med * 1e-3) * 1e-12, note))
for g in handles:
    g.close()
