"""Ring mode of the fused long-block kernel: a workgroup of 8 steady runs x 2 channels takes the packets of its chunk interleaved
(slot j: every 8th packet) and hands each packet's overlap carry to the next slot through LDS. A packet's output does not depend on
which wave computed the packet in front of it, so every run length — ring chunks of any size, groups that straddle segments or hold a
mixed run (the per-run fallback) — gives the same bits; and the oracle's PCM within the usual bar."""
import numpy as np
import pytest

from oracle import oracle_binding as ob
from parseoggvorbis_amd import binding
from parseoggvorbis_amd.binding import SetupSpec
from tests import synth_model
from tests.workloads import concat_batches as _concat, fixture_like_spec, synth_batch

pytestmark = pytest.mark.gpu
TOL = 1e-5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _spec(kind):
    """'coupled' (magnitude 0, angle 1), 'swapped' (magnitude 1, angle 0), 'uncoupled' stereo, or 'mono'."""
    if kind == "mono":
        return fixture_like_spec(1)
    f = fixture_like_spec(2)
    coup = {"coupled": [(0, 1)], "swapped": [(1, 0)], "uncoupled": []}[kind]
    return SetupSpec(2, f.blocksize0, f.blocksize1, f.floors, [(coup, [0, 0]), (coup, [1, 1])], [(0, 0), (1, 1)])


def _submit(spec, b, run_len, monkeypatch, want_taps=False):
    if run_len:
        monkeypatch.setenv("VSYN_RUN_LEN", str(run_len))
    else:
        monkeypatch.delenv("VSYN_RUN_LEN", raising=False)
    gpu = binding.Synth(spec, max_streams=len(b["segments"]))
    got = gpu.submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"], want_taps=want_taps)
    monkeypatch.delenv("VSYN_RUN_LEN", raising=False)
    return got


def _check(got, want, spec=None, b=None):
    """spec, b: also the per-packet gate against the float64 model of batch b (synth_model.py)."""
    assert got["rc"] == want["rc"] == 0, (got["rc"], got["flags"], want["rc"])
    assert np.array_equal(got["emit_len"], want["emit_len"])
    scale = max(1.0, float(np.abs(want["pcm"]).max()))
    assert float(np.abs(got["pcm"] - want["pcm"]).max()) < TOL * scale
    if b is not None:
        synth_model.check_model(got, spec, b)


# segment lengths: shorter than one round of slots (1-7), one round, chunks that 8R does not divide, several chunks
LENGTHS = [1, 2, 3, 5, 7, 8, 9, 23, 40, 97, 130]
RUN_LENS = [3, 5, 8, 0]  # 0: the planned run length


@pytest.mark.parametrize("kind", ["coupled", "swapped", "uncoupled", "mono"])
def test_ring_chunks_every_length_same_bits_for_every_run_length(kind, monkeypatch):
    spec = _spec(kind)
    b = _concat([synth_batch(spec, 1, n, "long", seed=50 + n, unused_frac=0.15, granule_last=True) for n in LENGTHS])
    want = ob.OracleSynth(spec, len(b["segments"])).submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"])
    ref = None
    for rl in RUN_LENS:
        got = _submit(spec, b, rl, monkeypatch)
        _check(got, want, spec, b)
        if ref is None:
            ref = got
        else:
            assert np.array_equal(bits(got["pcm"]), bits(ref["pcm"])), rl


@pytest.mark.parametrize("at", [0, 3, 21, 62])
def test_group_with_one_mixed_run_falls_back_with_the_same_bits(at, monkeypatch):
    """One short block among long ones: its run (and so its group of 8 runs) takes the per-run path, the other groups the ring."""
    spec = _spec("coupled")
    npk = 96
    flags = np.ones(npk, np.uint8)
    flags[at] = 0
    b = _concat([synth_batch(spec, 1, npk, flags, seed=7 + at, granule_last=True),
                 synth_batch(spec, 2, npk, "long", seed=8 + at, granule_last=True)])
    want = ob.OracleSynth(spec, len(b["segments"])).submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"])
    ref = None
    for rl in RUN_LENS:
        got = _submit(spec, b, rl, monkeypatch)
        _check(got, want, spec, b)
        if ref is None:
            ref = got
        else:
            assert np.array_equal(bits(got["pcm"]), bits(ref["pcm"])), rl


@pytest.mark.parametrize("run_len", RUN_LENS)
def test_stream_cut_across_submits_equals_the_uncut_submit(run_len, monkeypatch):
    """A carry-in makes the first run of the later submits a mixed-path run (its group falls back); the rest of the stream runs in
    rings. Cut == uncut, bit for bit."""
    spec = _spec("coupled")
    npk = 150
    b = synth_batch(spec, 1, npk, "long", seed=77, unused_frac=0.1)
    one = _submit(spec, b, run_len, monkeypatch)
    total = int(one["emit_len"].sum())
    off = np.arange(npk + 1) * spec.channels * (spec.blocksize1 // 2)
    if run_len:
        monkeypatch.setenv("VSYN_RUN_LEN", str(run_len))
    gpu = binding.Synth(spec, max_streams=2)
    monkeypatch.delenv("VSYN_RUN_LEN", raising=False)
    parts = []
    cuts = [0, 1, 9, 70, 71, 150]
    for a, e in zip(cuts[:-1], cuts[1:]):
        seg = b["segments"].copy()
        seg["stream"], seg["first_packet"], seg["num_packets"], seg["flags"], seg["residue_off"] = 1, 0, e - a, 1 if a == 0 else 0, 0
        r = gpu.submit_host(b["packets"][a:e], seg, b["ys"][a:e], b["residue"][off[a]:off[e]], b["plane_stride"])
        assert r["rc"] == 0
        assert np.array_equal(r["emit_len"], one["emit_len"][a:e])
        parts.append(r["pcm"][0][:, :int(r["emit_len"].sum())])
    got = np.concatenate(parts, axis=1)
    assert np.array_equal(bits(got), bits(one["pcm"][0][:, :total]))


@pytest.mark.parametrize("run_len", [3, 0])
def test_feature_tap_kernel_in_ring_mode(run_len, monkeypatch):
    spec = _spec("coupled")
    b = _concat([synth_batch(spec, 1, n, "long", seed=90 + n, unused_frac=0.2, granule_last=True) for n in (5, 40, 97)])
    want = ob.OracleSynth(spec, len(b["segments"])).submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"],
                                                                want_taps=True)
    got = _submit(spec, b, run_len, monkeypatch, want_taps="features")
    _check(got, want, spec, b)
    assert np.array_equal(got["taps"]["floor_curve"], want["taps"]["floor_curve"])
    assert np.array_equal(got["taps"]["floor_final"], want["taps"]["floor_final"])
    plain = _submit(spec, b, run_len, monkeypatch)
    assert np.array_equal(bits(plain["pcm"]), bits(got["pcm"]))
