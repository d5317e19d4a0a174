"""The tuning estimation timed with device events (profiles/tuning_bench.txt): 64 mono segments of 10 s at 22 050 Hz,
n_fft 2048, hop 512. Cases, alternated in one process, three warm-up rounds and ten timed ones each:
  lin_power              the yardstick: the same FFT pass, its rows stored
  piptrack               vsyn_piptrack_device: the FFT pass, the peak pick, two dense rows stored
  tuning                 vsyn_tuning_device: the FFT pass, the peak pick into records, the reduction
  chroma tuning=0.0      vsyn_spectral_chroma_device at power 2, the parent's kernel
  tuning at power 2      vsyn_tuning_device at the chroma call's power
and, on the PCM of one host submit of 64 stereo streams of 215 long blocks (10 s at 22 050 Hz, a synthesis batch: broadband), the two
synchronous host entries by the wall clock, rows copied back, two warm-up calls and ten timed ones, one case after the other:
  chroma host tuning=0.0    vsyn_pcm_chain_chroma_host
  chroma host estimate      vsyn_pcm_chain_chroma_est_host: the estimate, the read-back, one filterbank per (rate, tuning) pair built
                            on the host (the first call builds them, the timed calls find them kept), the chroma kernels
  chroma host estimate, banks rebuilt   the same with the kept filterbanks dropped before every call (another n_chroma in between)
Prints the medians and the ratios. Run from the repository root with PYTHONPATH set to it; under rocprofv3 --kernel-trace --stats --
python profiles/tuning_bench.py for the kernels' own times. Does not touch bench.py."""
import ctypes as C
import time

import numpy as np
import torch

from parseoggvorbis_amd import spectral, tuning
from parseoggvorbis_amd.binding import Synth
from tests import tuning_model as tm
from tests.workloads import fixture_like_spec, synth_batch

S, T, SR, N, HOP = 64, 220500, 22050, 2048, 512
g = Synth(fixture_like_spec(2), device=0, max_streams=4)
x = np.stack([tm.chord(T, SR, 0.01 * (i - 32), seed=i) for i in range(S)])
d_pcm = torch.from_numpy(x).cuda()
d_frames = torch.full((S,), T, dtype=torch.int32, device="cuda")
lin = spectral.spectral_spec("lin_power", n_fft=N, hop_length=HOP, power=1)
lin2 = spectral.spectral_spec("lin_power", n_fft=N, hop_length=HOP, power=2)
chroma = spectral.spectral_spec("chroma", n_fft=N, hop_length=HOP, power=2)
tun = tuning.tuning_spec()
F = int(g.lib.vsyn_spectral_num_frames(C.byref(lin), T))
NB = N // 2 + 1
d_a = torch.zeros((S * F + 8) * NB, dtype=torch.float32, device="cuda")
d_b = torch.zeros((S * F + 8) * NB, dtype=torch.float32, device="cuda")
d_t = torch.zeros(S, dtype=torch.float64, device="cuda")
d_c = torch.zeros((S, 2), dtype=torch.int64, device="cuda")
st = torch.cuda.current_stream().cuda_stream
rates = [SR] * S
args = (rates, d_pcm.data_ptr(), T, 1, d_frames.data_ptr())


cases = [("lin_power", lambda: g.spectral_device(lin, *args, d_a.data_ptr(), None, st)),
         ("piptrack", lambda: g.piptrack_device(lin, tun, *args, d_a.data_ptr(), d_b.data_ptr(), None, st)),
         ("tuning", lambda: g.tuning_device(lin, tun, *args, d_t.data_ptr(), d_c.data_ptr(), st)),
         ("chroma tuning=0.0", lambda: g.spectral_chroma_device(chroma, None, *args, d_a.data_ptr(), None, st)),
         ("tuning at power 2", lambda: g.tuning_device(lin2, tun, *args, d_t.data_ptr(), d_c.data_ptr(), st))]
ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in cases]
times = [[] for _ in cases]
for it in range(13):
    for i, (_, run) in enumerate(cases):
        ev[i][0].record()
        run()
        ev[i][1].record()
    torch.cuda.synchronize()
    if it >= 3:
        for i in range(len(cases)):
            times[i].append(ev[i][0].elapsed_time(ev[i][1]))
med = {}
for (name, _), t in zip(cases, times):
    med[name] = float(np.median(t))
    print("%s: median of 10 %.3f ms (min %.3f, max %.3f) for %d segments of %d frames" % (name, med[name], min(t), max(t), S, F))
t, c = d_t.cpu().numpy(), d_c.cpu().numpy()
print("tuning / lin_power %.2f; piptrack / lin_power %.2f; (chroma + tuning at power 2) / chroma %.2f"
      % (med["tuning"] / med["lin_power"], med["piptrack"] / med["lin_power"],
         (med["chroma tuning=0.0"] + med["tuning at power 2"]) / med["chroma tuning=0.0"]))
print("peaks per segment: median %d, selected %d; estimates %.2f .. %.2f" % (np.median(c[:, 0]), np.median(c[:, 1]), t.min(), t.max()))
g.close()

# the host entries, on a submit's PCM
setup = fixture_like_spec(2)
b = synth_batch(setup, streams=S, packets_per_stream=216, pattern="long", seed=9)
h = Synth(setup, device=0, max_streams=S)
assert h.submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"], flags=4)["rc"] == 0  # KEEP_PCM
other = spectral.chroma_spec(n_chroma=13)


def host(est, drop=False):
    if drop:
        h.pcm_chain_chroma_host(None, False, None, None, spectral.spectral_spec("chroma", n_fft=64, hop_length=4096), other, None, None, rates)
    t0 = time.perf_counter()
    r = h.pcm_chain_chroma_est_host(None, False, None, None, chroma, None, None, None, est, rates)
    return 1e3 * (time.perf_counter() - t0), r


hcases = [("chroma host tuning=0.0", None, False), ("chroma host estimate", tun, False), ("chroma host estimate, banks rebuilt", tun, True)]
htimes = [[] for _ in hcases]
for i, (_, est, drop) in enumerate(hcases):  # one case after the other: a handle keeps the filterbanks of its last call
    for it in range(12):
        ms, r = host(est, drop)
        if it >= 2:
            htimes[i].append(ms)
        if est is not None:
            pairs = len(set(r["tuning"].tolist()))
hmed = []
for (name, _, _), tms in zip(hcases, htimes):
    hmed.append(float(np.median(tms)))
    print("%s: median of 10 %.3f ms (min %.3f, max %.3f), %d rows of 12" % (name, hmed[-1], min(tms), max(tms), int(r["seg_rows"].sum())))
print("estimate / tuning=0.0 %.2f (banks kept), %.2f (banks rebuilt); %d distinct tunings among %d segments"
      % (hmed[1] / hmed[0], hmed[2] / hmed[0], pairs, S))
h.close()
