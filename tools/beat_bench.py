"""The beat stage next to the onset and tempogram stages (profiles/beat_bench.txt): 256 segments of F = 2584 frames (60 s
at 22050 / 512), 128 columns: onset strength, the tempogram mean at W = 344 (ac_size 8 s), the beat stage at P = 22. Three warm-up rounds
and ten timed ones; prints the device events' medians. Run from the repository root with PYTHONPATH set to it, under
rocprofv3 --kernel-trace --stats -- python tools/beat_bench.py for the kernels' own times."""
import numpy as np
import torch

from parseoggvorbis_amd import binding
from parseoggvorbis_amd.binding import Synth
from tests import rhythm_model as rm
from tests.workloads import fixture_like_spec

S, F, D, P, W = 256, 2584, 128, 22, 344
g = Synth(fixture_like_spec(2), device=0, max_streams=4)
rows = np.concatenate([rm.rows(F, D, 100 + (i % 8)) for i in range(S)])
d_rows = torch.from_numpy(rows).cuda()
d_env = torch.zeros(S * F + 8, dtype=torch.float32, device="cuda")
d_mean = torch.zeros(S * W + 8, dtype=torch.float64, device="cuda")
d_beats = torch.zeros(S * F + 8, dtype=torch.int32, device="cuda")
d_cnt = torch.zeros(S + 1, dtype=torch.int32, device="cuda")
d_ref = torch.zeros(S + 1, dtype=torch.int32, device="cuda")
st = torch.cuda.current_stream().cuda_stream
onset = binding.OnsetSpec(1, 1, 2048, 512, 1)
tg = binding.TempogramSpec(0, 512, 3, 0, 8.0)
beat = binding.BeatSpec(100.0, 120.0, 0.0, 512, 1)
seg = [F] * S
ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
times = []
for it in range(13):
    ev[0].record()
    g.onset_strength_device(onset, D, seg, d_rows.data_ptr(), d_env.data_ptr(), st)
    ev[1].record()
    g.tempogram_device(tg, seg, [22050] * S, d_env.data_ptr(), None, d_mean.data_ptr(), st)
    ev[2].record()
    g.beat_track_device(beat, seg, [P] * S, d_env.data_ptr(), d_beats.data_ptr(), d_cnt.data_ptr(), d_ref.data_ptr(), stream=st)
    ev[3].record()
    torch.cuda.synchronize()
    if it >= 3:
        times.append([ev[k].elapsed_time(ev[k + 1]) for k in range(3)])
t = np.median(np.array(times), axis=0)
cnt = d_cnt.cpu().numpy()[:S]
print("events, median of 10 (ms): onset %.4f tempogram mean %.4f beats %.4f; beats per segment %d..%d" % (t[0], t[1], t[2], cnt.min(), cnt.max()))
g.close()
