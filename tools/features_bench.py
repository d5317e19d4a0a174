"""Feature-matrix throughput: 65 536 stereo packets at 256/2048 (64 streams x 1024 packets, the fixtures' setup), each kind,
through vsyn_features_host (host staging + kernels + copy back) and, timed with HIP events by torch, the device part alone
(vsyn_features_device on resident inputs). Prints one JSON line per kind: M rows/s. Run under rocprofv3 --kernel-trace --stats
for the per-kernel split.
Usage: python tools/features_bench.py [--steps 20]"""
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

from parseoggvorbis_amd import features  # noqa: E402
from parseoggvorbis_amd.binding import Synth, VsynError  # noqa: E402
from tests.workloads import fixture_like_spec, synth_batch  # noqa: E402

CASES = [("floor_final_ys", 30, {}), ("floor_final_ys_rendered", 30, {}), ("residue_ys", 30, {}),
         ("residue_ys_with_floor", 30, {"log1p_abs_space": True})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    spec = fixture_like_spec(2)
    b = synth_batch(spec, streams=64, packets_per_stream=1024, pattern="long", seed=5)
    s = Synth(spec, device=0, max_streams=64)
    P, S = len(b["packets"]), len(b["segments"])
    dev = torch.device("cuda:0")
    d_pk = torch.from_numpy(b["packets"].view(np.uint8).copy()).to(dev)
    d_seg = torch.from_numpy(b["segments"].view(np.uint8).copy()).to(dev)
    d_ys = torch.from_numpy(b["ys"].astype(np.int16).copy()).to(dev)
    d_res = torch.from_numpy(b["residue"]).to(dev)
    d_off = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev)
    for kind, dim, kw in CASES:
        fs = features.feature_spec(dim, kind, **kw)
        r = s.features_host(fs, b["packets"], b["segments"], b["ys"], b["residue"])
        rows = r["rows"].shape[0]
        t0 = time.perf_counter()
        for _ in range(a.steps):
            s.features_host(fs, b["packets"], b["segments"], b["ys"], b["residue"])
        host_ms = (time.perf_counter() - t0) / a.steps * 1e3
        d_rows = torch.empty((rows, dim), dtype=torch.float32, device=dev)
        err = C.c_char_p()

        def run():
            rc = s.lib.vsyn_features_device(s.h, C.byref(fs), P, d_pk.data_ptr(), S, d_seg.data_ptr(), 1024, d_ys.data_ptr(), d_res.data_ptr(),
                                            d_rows.data_ptr(), d_off.data_ptr(), C.c_void_p(stream.cuda_stream), C.byref(err))
            if rc:
                raise VsynError(rc, (err.value or b"").decode())
        run()
        torch.cuda.synchronize()
        assert np.array_equal(d_rows.cpu().numpy(), r["rows"])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.steps):
            run()
        e1.record(stream)
        torch.cuda.synchronize()
        dev_ms = e0.elapsed_time(e1) / a.steps
        print(json.dumps(dict(kind=kind, output_dim=dim, packets=P, rows=rows, host_call_ms=round(host_ms, 3), device_ms=round(dev_ms, 4),
                              device_mrows_per_s=round(rows / dev_ms / 1e3, 1), host_mrows_per_s=round(rows / host_ms / 1e3, 1))))
    s.close() if hasattr(s, "close") else None


if __name__ == "__main__":
    main()
