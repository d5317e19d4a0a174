"""The resampler's index arithmetic (csrc/vsyn_resample.h) on the device at the shapes of tests/resample_cases.py, against
tests/resample_model.py: every case through vsyn_resample_device on caller buffers (NaN-filled output with guards in front and
behind, -1-filled out_frames), once with impulses and once with noise; and vsyn_pcm_resample_host on a multi-chunk global pair and
the pairs at the LDS budget. Gates: resample_cases (one float32 ulp of the tap for an impulse, exactly 0 where none reaches; 2e-6
max(1, max|x|) for noise at K4 <= 64, the chain bound B_j above). tests/test_resample_cases_cpu.py shows that each case reaches the
variant, chunk, edge and crossing it names; no test can read back which variant ran.

Built to catch:
    a 32-bit c0, qb, a0 or e                          long_lds (LDS variant), long_global (global): impulses and noise under tiles
                                                      whose c0 is 2^32 or more, zeros everywhere else
    rs_span4 short by one float4                      widest_span (22050 -> 16000, tile 4), budget_lds (380 -> 31, tile 0), and the
                                                      44100 -> 16000 segments past one tile: the last input of the tile's span
                                                      carries an impulse, and the noise reaches it
    a dynamic-LDS limit below the launch size         budget_lds: 380 -> 31 needs exactly RS_LDS_BUDGET, the limit the host sets: the
                                                      launch would fail; budget_global (204 -> 13, 16 bytes more) next to it
    chunk-local j, jend off by one                    edges: T_out 1023 .. 16385 under all three variants, sentinels behind T_out
    the fast path of <false> at its borders           edges, pitch_pair, up_65536_near, budget_global: i0 = K4 - 1 and i0 = T - 1
                                                      lie in the first and in the third chunk; impulses at 0 and T - 1
    staging that reads past T or before 0, unaligned  align_*: NaN behind T, impulses at 0 and T - 1, bit-identical to the aligned run
    the binary search on equal offsets, scan pass 2   many_segments: S = 700, empty and skipped segments between the others
None of these breaks was tried on a device. The first, second and fourth were tried on a numpy restatement of the kernel's tile loop
(tests/test_resample_cases_cpu.py, test_the_checks_catch_the_breaks_on_an_emulated_kernel), which passes these checks as written and
fails them with the break. `<` for `<=` alone would pass here (the pair would take the global variant, which gives the same bits);
the CPU module reads that line in the header.
"""
import time

import numpy as np
import pytest

from tests import resample_cases as rc
from tests import resample_model as rm

pytestmark = pytest.mark.gpu
GUARD = 64  # floats of NaN in front of and behind the output (256 bytes: the offsets stay what the case says)
_RUNS = {}


@pytest.fixture(scope="module")
def synth():
    import torch
    assert torch.cuda.is_available()
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    yield g
    g.close()


class Buffers:
    """The case's input at its pointer offset, its frames, and a NaN-filled output at its offset between two guards."""

    def __init__(self, case, x, frames=None):
        import torch
        self.case, (self.S, self.C, self.plane) = case, x.shape
        self.op = rc.out_plane(case)
        self.d_in = torch.full((case["in_off"] + x.size + 4,), float("nan"), dtype=torch.float32, device="cuda")
        self.d_in[case["in_off"]:case["in_off"] + x.size].copy_(torch.from_numpy(x.reshape(-1)))
        self.d_frames = torch.tensor(case["frames"] if frames is None else frames, dtype=torch.int32, device="cuda")
        self.in_ptr = self.d_in.data_ptr() + 4 * case["in_off"]
        assert self.d_in.data_ptr() % 256 == 0

    def output(self):
        import torch
        d_out = torch.full((GUARD + self.case["out_off"] + self.S * self.C * self.op + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        d_of = torch.full((self.S,), -1, dtype=torch.int32, device="cuda")
        assert d_out.data_ptr() % 256 == 0
        return d_out, d_of, d_out.data_ptr() + 4 * (GUARD + self.case["out_off"])

    def fetch(self, d_out, d_of):
        import torch
        torch.cuda.synchronize()
        flat = d_out.cpu().numpy()
        a = GUARD + self.case["out_off"]
        assert np.isnan(flat[:a]).all() and np.isnan(flat[a + self.S * self.C * self.op:]).all(), "a write outside the output"
        return flat[a:a + self.S * self.C * self.op].reshape(self.S, self.C, self.op), d_of.cpu().numpy()

    def run(self, synth):
        import torch
        d_out, d_of, out_ptr = self.output()
        synth.resample_device(self.case["in_rates"], self.case["out_rate"], self.in_ptr, self.plane, self.C, self.d_frames.data_ptr(), out_ptr,
                              self.op, d_of.data_ptr(), torch.cuda.current_stream().cuda_stream)
        return self.fetch(d_out, d_of)


def device_run(synth, name, cls):
    """(x, y, out_frames) of the case under the input class; kept for the cases that more than one test reads."""
    if (name, cls) in _RUNS:
        return _RUNS[name, cls]
    case = rc.BY_NAME[name]
    x = rc.impulse_input(case) if cls == "impulses" else rc.noise_input(case)
    res = (x,) + Buffers(case, x).run(synth)
    if name.startswith("align_") or name in ("many_segments", "frames_past_plane"):  # the cases that a second test compares
        _RUNS[name, cls] = res
    return res


def check_case(case, cls, x, y, of):
    """Frames, sentinels and every plane of every segment against the model. Returns {gate: the worst |d| / gate}."""
    worst = {}
    skip = rc.footprint(case["in_rates"][0], case["out_rate"], case["plane"], case["stretch"][0], sum(case["stretch"])) if case["stretch"] else None
    for g, r in enumerate(case["in_rates"]):
        T, To = rc.seg_frames(case, g), rc.seg_out_frames(case, g)
        assert of[g] == To, (case["name"], g, r, of[g], To)
        assert np.isnan(y[g, :, To:]).all(), (case["name"], g, "written past T_out")
        if not r:
            continue
        planes = rc.impulse_planes(case, g)
        for c in range(case["channels"]):
            what = (case["name"], cls, g, r, c)
            if cls == "noise" or rc.plan(r, case["out_rate"])["variant"] == "copy":
                w, kind = rc.check_noise(y[g, c, :To], x[g, c, :T], r, case["out_rate"], what)
            else:
                w, kind = rc.check_impulses(y[g, c, :To], r, case["out_rate"], T, planes[c], what, skip if (g, c) == (0, 0) else None), "tap"
                if skip and (g, c) == (0, 0):
                    j = np.arange(skip[0], skip[1], dtype=np.int64)
                    ws, _ = rc.check_noise(y[g, c, skip[0]:skip[1]], x[g, c, :T], r, case["out_rate"], what, j=j)
                    worst["flat"] = max(worst.get("flat", 0.0), ws)
            worst[kind] = max(worst.get(kind, 0.0), w)
    return worst


@pytest.mark.parametrize("name", rc.IDS)
def test_case_against_the_model(synth, name):
    """Every case, impulses then noise (long_lds: its one input): out_frames exact, NaN behind every T_out and around the output,
    every plane inside its gate. Prints the worst ratio to each gate."""
    case = rc.BY_NAME[name]
    for cls in ("impulses",) if case["stretch"] else ("impulses", "noise"):
        t0 = time.time()
        x, y, of = device_run(synth, name, cls)
        t1 = time.time()
        worst = check_case(case, cls, x, y, of)
        print("%s %s: worst |d| / gate %s (device and copies %.2f s, model %.2f s)"
              % (name, cls, ", ".join("%s %.3g" % kv for kv in sorted(worst.items())), t1 - t0, time.time() - t1))


def test_unaligned_runs_are_the_aligned_run(synth):
    """Plane strides 4k, 4k + 1, 4k + 2 by pointer offsets 0 to 3 on input and output: the same bits as the run that is aligned
    throughout, so the scalar staging path gives what the 16-byte one gives (each is also held to the model above)."""
    for cls in ("impulses", "noise"):
        x0, y0, of0 = device_run(synth, rc.ALIGNED, cls)
        for case in rc.CASES:
            if case["name"].startswith("align_") and case["name"] != rc.ALIGNED:
                x, y, of = device_run(synth, case["name"], cls)
                T = max(case["frames"])
                assert np.array_equal(x[:, :, :T].view(np.uint32), x0[:, :, :T].view(np.uint32))  # the same input: the seed is the case's
                n = int(of0.max())
                assert np.array_equal(of, of0) and np.array_equal(y[:, :, :n].view(np.uint32), y0[:, :, :n].view(np.uint32)), (case["name"], cls)


def test_many_segments_are_position_independent(synth):
    """S = 700: every segment of the batch is bit for bit the same segment resampled alone (one call per segment on the same
    device buffers, S = 1), out_frames included; a skipped segment leaves its output alone."""
    import torch
    case = rc.BY_NAME["many_segments"]
    x, y, of = device_run(synth, "many_segments", "noise")
    b = Buffers(case, x)
    d_out, d_of, out_ptr = b.output()
    s = torch.cuda.current_stream().cuda_stream
    for g, r in enumerate(case["in_rates"]):
        if r:
            synth.resample_device([r], case["out_rate"], b.in_ptr + 4 * g * b.C * b.plane, b.plane, b.C, b.d_frames.data_ptr() + 4 * g,
                                  out_ptr + 4 * g * b.C * b.op, b.op, d_of.data_ptr() + 4 * g, s)
    y1, of1 = b.fetch(d_out, d_of)
    run = np.array(case["in_rates"]) != 0
    assert np.array_equal(of1[run], of[run]) and (of1[~run] == -1).all() and (of[~run] == 0).all()
    assert np.array_equal(y1.view(np.uint32), y.view(np.uint32))


def test_frames_above_the_plane_are_the_plane(synth):
    case = rc.BY_NAME["frames_past_plane"]
    for cls in ("impulses", "noise"):
        x, y, of = device_run(synth, "frames_past_plane", cls)
        y1, of1 = Buffers(case, x, frames=[case["plane"]] * len(case["frames"])).run(synth)
        assert np.array_equal(of, of1) and np.array_equal(y.view(np.uint32), y1.view(np.uint32))
        assert of.tolist() == [rm.num_frames(r, case["out_rate"], case["plane"]) for r in case["in_rates"]]


def _pcm_s16(x):
    return np.clip(np.rint(np.float32(x) * np.float32(32768.0)), -32768, 32767).astype(np.int64)


def test_host_form_on_a_multi_chunk_global_pair_and_at_the_budget():
    """vsyn_pcm_resample_host behind a submit of known PCM (vsyn_pcm_fetch_host gives it): 37084 -> 44100 (global, several chunks
    per segment), 380 -> 31 (LDS at the budget) and 204 -> 13 (global, 16 bytes above it); float32 against the model by the pair's
    gate, int16 within 1 LSB of the model's int16."""
    from parseoggvorbis_amd.binding import Synth, VSYN_PCM_F32, VSYN_PCM_S16
    from tests.workloads import fixture_like_spec, synth_batch
    spec = fixture_like_spec(2)
    b = synth_batch(spec, streams=2, packets_per_stream=16, pattern="long", seed=41)
    S = len(b["segments"])
    g = Synth(spec, device=0, max_streams=4)
    assert g.submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"], flags=4)["rc"] == 0  # KEEP_PCM
    pcm, frames = g.pcm_fetch_host(VSYN_PCM_F32, S, b["plane_stride"])
    for r_in, r_out, chunks in ((37084, 44100, 2), (380, 31, 1), (204, 13, 1)):
        y, fo = g.pcm_resample_host([r_in] * S, r_out, VSYN_PCM_F32)
        y16, fo16 = g.pcm_resample_host([r_in] * S, r_out, VSYN_PCM_S16)
        assert np.array_equal(fo, fo16)
        worst = {}
        for gi in range(S):
            x = np.ascontiguousarray(pcm[gi, :frames[gi]].T)
            To = rm.num_frames(r_in, r_out, int(frames[gi]))
            assert fo[gi] == To and -(-To // rc.RS_CHUNK) >= chunks, (r_in, gi, To)
            assert not y[gi, :, To:].any() and not y16[gi, To:].any()
            for c in range(x.shape[0]):
                w, kind = rc.check_noise(np.ascontiguousarray(y[gi, c, :To]), x[c], r_in, r_out, ("host", r_in, gi, c))
                worst[kind] = max(worst.get(kind, 0.0), w)
            want16 = _pcm_s16(rm.resample_at(x, r_in, r_out, np.arange(To), P=rc.tables(r_in, r_out)[1])).T
            assert np.abs(y16[gi, :To].astype(np.int64) - want16).max(initial=0) <= 1, (r_in, gi)
        print("host %d -> %d: worst |d| / gate %s" % (r_in, r_out, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    g.close()
