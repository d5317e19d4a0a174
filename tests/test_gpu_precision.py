"""Synthesis PCM per packet against the float64 model of synth_model.py, on every kernel path and on content that probes precision:
quiet (peak about 5e-5), loud (floors 150..250, residue x 1000: |x| about 1e5), a quiet and a loud stream in one submit (about 1e6
apart), loud and quiet packets alternating within a segment (carries from loud blocks into quiet ones, across ring slots too), dense
Gaussian residue, and silent channels (floor unused, residue zero) in front of and behind loud blocks, which must come out exactly 0
where both contributing blocks are zero. Gate: max |got - model| <= G * 2^-24 * s[p, c] per packet and channel (synth_model.py;
the oracle passes the same gate on the same batches, test_synth_model_cpu.py). Every case reads back from the kernel profile which
synthesis kernel ran. The worst ratio per kernel path and profile is printed at the end."""
import numpy as np
import pytest

from oracle import oracle_binding as ob
from parseoggvorbis_amd import binding
from parseoggvorbis_amd.binding import SetupSpec
from tests import synth_model as sm
from tests.test_gpu_damaged_files import ring_planned
from tests.workloads import fixture_like_spec, loudness_profiles as profiles, synth_batch

pytestmark = pytest.mark.gpu
PRE = binding.VSYN_SUBMIT_PRE_KERNELS
HIDDEN_PRE = binding.VSYN_SUBMIT_INPUTS_READY | binding.VSYN_SUBMIT_PRE_KERNELS
STAGED = binding.VSYN_SUBMIT_STAGED
PREPS = [0, PRE, HIDDEN_PRE]
KERNEL = dict(tuned="vsyn_fused_kernel", generic="vsyn_fused_u_kernel", staged="staged")
WORST = {}


def _note(path, profile, ratio):
    WORST[(path, profile)] = max(WORST.get((path, profile), 0.0), ratio)


def _synth(spec, streams, run_len=None, monkeypatch=None):
    if run_len:
        monkeypatch.setenv("VSYN_RUN_LEN", str(run_len))
    g = binding.Synth(spec, max_streams=streams)
    if run_len:
        monkeypatch.delenv("VSYN_RUN_LEN")
    g.profile(1)
    return g


def _run(g, spec, b, kind, flags=0, profile="", path=None):
    """One submit on g, the kernel that ran asserted, the per-packet gate applied; -> worst ratio."""
    g.reset()
    got = g.submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"], flags=flags)
    _, launches, kernel = g.profile_read()
    ctx = (kind, flags, profile, g.fused_paths, launches, kernel)
    assert got["rc"] == 0 and got["flags"] == 0, ctx
    assert launches and KERNEL[kind] in kernel, ctx
    if kind != "staged":
        assert g.fused_paths & 3, ctx  # the setup gets a fused kernel (long runs, and mixed runs on the size-generic one)
    r = sm.check_model(got, spec, b, ctx=ctx)
    _note(path or kind, profile, r)
    return r


def _paths(kind):
    return [(kind, f) for f in PREPS] + [("staged", STAGED)]


@pytest.mark.parametrize("coupled", [True, False])
def test_tuned_kernel_every_profile_and_preparation(coupled):
    """The tuned 256/2048 kernel: mixed runs and long runs (quiet / alternate profiles in both), every preparation, and the staged
    kernels on the same batches."""
    spec = fixture_like_spec(2, 256, 2048, coupled=coupled)
    pr = profiles(spec, npk=40)
    pr["long_alternate"] = synth_batch(spec, 2, 40, "long", seed=31, alternate=1, granule_last=True)
    pr["long_quiet"] = synth_batch(spec, 2, 40, "long", seed=32, ylo=0, yhi=8)
    g = _synth(spec, 3)
    for name, b in pr.items():
        for kind, flags in _paths("tuned"):
            _run(g, spec, b, kind, flags, name, path="%s/%d" % (kind, flags))


def _ring_batches(spec):
    out = dict(alternate=synth_batch(spec, 1, 97, "long", seed=61, alternate=1, granule_last=True),
               quiet=synth_batch(spec, 1, 97, "long", seed=62, ylo=0, yhi=8),
               loud=synth_batch(spec, 1, 97, "long", seed=63, ylo=150, yhi=250, residue_scale=1000.0),
               gauss=synth_batch(spec, 1, 97, "long", seed=64, residue="gauss", alternate=5))
    sil = synth_batch(spec, 1, 97, "long", seed=65, alternate=2)
    from tests.workloads import silence
    out["silent"] = silence(spec, sil, [q for q in range(97) if q % 7 in (2, 3, 4)])
    flags = np.ones(96, np.uint8)
    flags[21] = 0  # one short block: its run and its group of 8 runs take the per-run fallback
    out["fallback"] = synth_batch(spec, 1, 96, flags, seed=66, alternate=1, granule_last=True)
    return out


@pytest.mark.parametrize("run_len", [3, 4])
def test_tuned_kernel_ring_mode(run_len, monkeypatch):
    spec = fixture_like_spec(2)
    g = _synth(spec, 1, run_len, monkeypatch)
    for name, b in _ring_batches(spec).items():
        d = dict(P=len(b["packets"]), packets=b["packets"])
        assert ring_planned(spec, d, run_len), name
        _run(g, spec, b, "tuned", 0, name, path="ring")


GENERIC = [(2, 128, 1024), (2, 512, 4096), (1, 64, 8192), (2, 4096, 4096), (1, 8192, 8192)]


@pytest.mark.parametrize("C,bs0,bs1", GENERIC)
def test_generic_kernel_every_profile(C, bs0, bs1):
    spec = fixture_like_spec(C, bs0, bs1, coupled=False)
    g = _synth(spec, 3)
    for name, b in profiles(spec, npk=16 if bs1 >= 4096 else 30).items():
        for kind, flags in [("generic", 0), ("generic", PRE), ("staged", STAGED)]:
            _run(g, spec, b, kind, flags, name, path="%s/%d/%d" % (kind, bs0, bs1))


@pytest.mark.parametrize("C,coup", [(3, [(0, 1), (1, 2)]), (6, [(0, 1), (0, 2), (3, 4), (4, 5)]),
                                    (16, [(2 * i, 2 * i + 1) for i in range(8)])])
def test_generic_kernel_chained_and_many_coupled_channels(C, coup):
    xs_s = [0, 64, 8, 32, 16, 48]
    xs_l = [0, 512] + [int(v) for v in np.random.default_rng(1).permutation(np.arange(1, 512))[:40]]
    spec = SetupSpec(C, 128, 1024, [(1, xs_s), (3, xs_l)], [(coup, [0] * C), (coup, [1] * C)], [(0, 0), (1, 1)])
    g = _synth(spec, 2)
    for name, kw in (("alternate", dict(alternate=1)), ("gauss", dict(residue="gauss")), ("quiet", dict(ylo=0, yhi=8))):
        b = synth_batch(spec, 2, 20, "mixed", seed=C, granule_last=True, **kw)
        for kind, flags in [("generic", 0), ("staged", STAGED)]:
            _run(g, spec, b, kind, flags, "%dch-%s" % (C, name))


@pytest.mark.parametrize("flags", [0, STAGED])
def test_stream_cut_across_submits(flags):
    """The carry stays on the device between submits: every part against a model handle that continues the stream alike."""
    spec = fixture_like_spec(2)
    b = synth_batch(spec, 1, 90, "mixed", seed=71, alternate=1, granule_last=True)
    n = np.where(b["packets"]["mode"] == 1, spec.blocksize1, spec.blocksize0)
    off = np.concatenate([[0], np.cumsum(n // 2 * spec.channels)])
    g = _synth(spec, 2)
    m = sm.SynthModel(spec, 2)
    cuts = [0, 1, 5, 17, 18, 33, 60, 61, 90]
    for a, e in zip(cuts[:-1], cuts[1:]):
        seg = b["segments"].copy()
        seg["stream"], seg["first_packet"], seg["num_packets"], seg["flags"], seg["residue_off"] = 1, 0, e - a, 1 if a == 0 else 0, 0
        args = (b["packets"][a:e], seg, b["ys"][a:e], b["residue"][off[a]:off[e]], b["plane_stride"])
        got = g.submit_host(*args, flags=flags)
        _, launches, kernel = g.profile_read()
        assert got["rc"] == 0 and launches and KERNEL["staged" if flags else "tuned"] in kernel, (a, e, kernel)
        want = m.submit_host(*args)
        _note("cut/%d" % flags, "alternate", sm.gate(got["pcm"], want, seg, got["emit_len"], ctx=(a, e)))


@pytest.mark.parametrize("flags", [binding.VSYN_SUBMIT_INPUTS_READY, HIDDEN_PRE])
def test_submit_device_on_device_buffers(flags):
    import torch
    spec = fixture_like_spec(2)
    g = _synth(spec, 3)
    stream = torch.cuda.current_stream().cuda_stream
    for name, b in (("alternate", synth_batch(spec, 3, 40, "mixed", seed=81, alternate=1)),
                    ("both", synth_batch(spec, 3, 40, "long", seed=82, floor_ranges=[(0, 8), (150, 250), (0, 8)]))):
        P, S = len(b["packets"]), len(b["segments"])
        d = dict(pk=torch.from_numpy(b["packets"].view(np.uint8)).cuda(), seg=torch.from_numpy(b["segments"].view(np.uint8)).cuda(),
                 ys=torch.from_numpy(b["ys"].astype(np.int16)).cuda(), res=torch.from_numpy(b["residue"]).cuda(),
                 pcm=torch.zeros((S, 2, b["plane_stride"]), device="cuda"), emit=torch.zeros(P, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        g.reset()
        g.submit_device(P, d["pk"].data_ptr(), S, d["seg"].data_ptr(), 40, d["ys"].data_ptr(), d["res"].data_ptr(),
                        d["pcm"].data_ptr(), b["plane_stride"], d["emit"].data_ptr(), None, flags, stream)
        fl, bad = g.sync_status(stream)
        assert fl == 0, (fl, bad)
        _, launches, kernel = g.profile_read()
        assert launches and KERNEL["tuned"] in kernel, kernel
        got = dict(pcm=d["pcm"].cpu().numpy(), emit_len=d["emit"].cpu().numpy().astype(np.uint32))
        _note("device/%d" % flags, name, sm.check_model(got, spec, b, ctx=name))


def test_vq_residue_path():
    """Residue from VQ entries on one synthetic_vq_spec setup: the model is fed the oracle's VQ output."""
    from tests.test_gpu_vq import _random_vq_batch
    from tests.workloads import synthetic_vq_spec
    spec = fixture_like_spec(2)
    vqs = synthetic_vq_spec(2, spec.blocksize1)
    pattern = [1, 1, 0, 0, 0, 1, 1, 1]
    pk, seg, vqp, cls, ent, res = _random_vq_batch(spec, vqs, 4, 30, pattern, seed=91)
    g = _synth(spec, 4)
    g.attach_vq(vqs)
    blocks = [pattern[q % len(pattern)] for q in range(30)]
    ys = synth_batch(spec, 4, 30, blocks, seed=92, alternate=1)["ys"]  # loud and quiet floors alternating, per the packets' modes
    plane = 30 * spec.blocksize1 // 2
    out = g.submit_host_vq(pk, seg, ys, vqp, cls, ent, res.size, plane)
    assert out["rc"] == 0, out
    assert np.array_equal(out["residue"].view(np.uint32), res.view(np.uint32))
    b = dict(packets=pk, segments=seg, ys=ys, residue=res, plane_stride=plane)
    _note("vq", "alternate", sm.check_model(out, spec, b))


@pytest.mark.parametrize("C,bs0,bs1,coup", [(2, 256, 2048, [(0, 1)]), (3, 128, 1024, [(0, 1), (1, 2)]), (2, 512, 4096, [(1, 0)])])
def test_staged_taps(C, bs0, bs1, coup):
    """after_envelope bit for bit against the oracle (couplings, chains, unused channels); pcm_after_mdct per block within
    G * 2^-24 * rms(block) of the float64 IMDCT of that envelope."""
    f = fixture_like_spec(C, bs0, bs1)
    spec = SetupSpec(C, bs0, bs1, f.floors, [(coup, [0] * C), (coup, [1] * C)], [(0, 0), (1, 1)])
    for name, kw in (("alternate", dict(alternate=1)), ("gauss", dict(residue="gauss", unused_frac=0.3)),
                     ("quiet", dict(ylo=0, yhi=8))):
        b = synth_batch(spec, 2, 20, "mixed", seed=C + bs1, **kw)
        want = ob.OracleSynth(spec, 2).submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"], want_taps=True)
        got = binding.Synth(spec, max_streams=2).submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"],
                                                             want_taps=True)
        assert got["rc"] == 0
        env = got["taps"]["after_envelope"]
        assert np.array_equal(env.view(np.uint32), want["taps"]["after_envelope"].view(np.uint32)), name
        from tests.workloads import packet_blocks
        n_of, off = packet_blocks(spec, b["packets"], b["segments"])
        worst = 0.0
        for n in np.unique(n_of):
            ps = np.flatnonzero(n_of == n)
            idx = off[ps][:, None] + np.arange(C * n // 2)[None, :]
            y = sm.imdct(int(n), env[idx].reshape(-1, n // 2))
            md = got["taps"]["pcm_after_mdct"][2 * idx[:, :1] + np.arange(C * n)[None, :]].reshape(-1, n)
            rms = np.sqrt(np.mean(y * y, axis=1))
            d = np.abs(md - y).max(axis=1)
            assert np.all((d <= sm.G * sm.ULP * rms) | ((rms == 0) & (d == 0))), (name, n)
            worst = max(worst, float(np.max(np.where(rms > 0, d / (sm.ULP * np.where(rms > 0, rms, 1)), 0))))
        _note("staged-taps", name, worst)
        _note("staged", name, sm.check_model(got, spec, b))


def test_zz_print_worst_per_path_and_profile():
    print("\nworst max|got - model| / (2^-24 s) per (path, profile), gate %g:" % sm.G)
    for k in sorted(WORST):
        print("  %-28s %-16s %.1f" % (k[0], k[1], WORST[k]))
    assert all(v <= sm.G for v in WORST.values())
