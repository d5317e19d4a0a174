"""The float64 synthesis model of synth_model.py and its per-packet gate, settled on the CPU: the FFT IMDCT against the oracle's
closed form, the model's frame counts against the oracle's, and the oracle itself (the reference's float32 arithmetic, pinned bit
for bit) inside the gate G on every synthetic shape of the parity suite, the loudness profiles of the precision suite, the
reference's two fixtures and the 20 synth_NN fixtures. Also: synth_batch's defaults give the batches they gave before its
precision probes were added."""
import hashlib

import numpy as np
import pytest

from oracle import oracle_binding as ob
from tests import synth_model as sm
from tests.test_gpu_parity import SHAPES
from tests.workloads import fixture_like_spec, load_golden, loudness_profiles as profiles, synth_batch

WORST = {}  # block size -> the oracle's worst ratio over this module's cases (printed by the last test)


def _note(ratio, n):
    for k, v in sm.worst_by_block_size(ratio, n).items():
        WORST[k] = max(WORST.get(k, 0.0), v)


def _oracle_in_gate(spec, b, ctx=None):
    want = ob.OracleSynth(spec, len(b["segments"])).submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"])
    assert want["rc"] == 0, (want["flags"], want["first_bad"])
    m = sm.model_of(spec, b)
    assert np.array_equal(m["emit_len"], want["emit_len"])
    r = sm.per_packet_error(want["pcm"], m, b["segments"])
    _note(r, m["n"])
    sm.gate(want["pcm"], m, b["segments"], ctx=ctx)
    return float(r.max())


@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024, 2048, 4096, 8192])
def test_fft_imdct_equals_the_closed_form(n):
    """Within 1e-12 of the row's rms of the closed form with its phase reduced exactly (integer arithmetic mod 4n). The oracle's
    orc_imdct_closed_form rounds the unreduced phase, up to 1.25 pi n, in float64, which alone costs it about n * 1e-16 per term
    (measured 5.6e-12 of the rms at 8192): against it the bar is 1e-12 * max(1, n / 1024) of the rms."""
    rng = np.random.default_rng(n)
    x = np.concatenate([rng.standard_normal((2, n // 2)), np.round(rng.laplace(0, 1.5, (1, n // 2)))]).astype(np.float32)
    got = sm.imdct(n, x)
    i, k = np.arange(n)[:, None], np.arange(n // 2)[None, :]
    exact = x.astype(np.float64) @ np.cos(np.pi * (((2 * i + 1 + n // 2) * (2 * k + 1)) % (4 * n)) / (2 * n)).T
    for r in range(len(x)):
        cf = np.zeros(n)
        ob.oracle().orc_imdct_closed_form(n, ob.p(x[r]), ob.p(cf))
        rms = np.sqrt(np.mean(cf * cf))
        assert np.abs(got[r] - exact[r]).max() <= 1e-12 * rms, (n, r)
        assert np.abs(got[r] - cf).max() <= 1e-12 * max(1, n // 1024) * rms, (n, r)


@pytest.mark.parametrize("n", [64, 2048, 8192])
def test_float64_window_is_the_oracles(n):
    bs0, bs1 = min(n, 256), n
    w = np.zeros(bs1, np.float32)
    for lng, prev, nxt in ((1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1), (0, 1, 1)):
        m = bs1 if lng else bs0
        ob.oracle().orc_window(bs0, bs1, lng, prev, nxt, ob.p(w))
        assert np.abs(sm.window(bs0, bs1, lng, prev, nxt) - w[:m]).max() <= 2.0 ** -23


@pytest.mark.parametrize("C,bs0,bs1,pattern,streams,npk", SHAPES)
def test_oracle_in_gate_on_the_parity_shapes(C, bs0, bs1, pattern, streams, npk):
    """Same batches as test_gpu_parity.test_synthetic_vs_oracle (granule trimming, unused channels): frame counts exact, PCM in G."""
    spec = fixture_like_spec(C, bs0, bs1)
    b = synth_batch(spec, streams, npk, pattern, seed=bs0 + bs1 + C, unused_frac=0.1, granule_last=True)
    _oracle_in_gate(spec, b)


PROFILE_SETUPS = [(2, 256, 2048), (2, 128, 1024), (2, 512, 4096), (1, 64, 8192), (2, 4096, 4096), (1, 8192, 8192)]


@pytest.mark.parametrize("C,bs0,bs1", PROFILE_SETUPS)
def test_oracle_in_gate_on_the_loudness_profiles(C, bs0, bs1):
    spec = fixture_like_spec(C, bs0, bs1, coupled=bs0 != 256)
    worst = {}
    for name, b in profiles(spec).items():
        worst[name] = _oracle_in_gate(spec, b, ctx=name)
    print("oracle, %d x %d/%d: worst per profile %s" % (C, bs0, bs1, {k: round(v, 1) for k, v in worst.items()}))


def test_profiles_have_the_intended_loudness():
    spec = fixture_like_spec(2, 256, 2048, coupled=False)
    pr = profiles(spec)
    peak = {k: float(np.abs(sm.model_of(spec, b)["pcm"]).max()) for k, b in pr.items()}
    assert 1e-5 < peak["quiet"] < 2e-4, peak
    assert peak["loud"] > 1e4, peak
    m = sm.model_of(spec, pr["both"])
    q, l = float(np.abs(m["pcm"][0]).max()), float(np.abs(m["pcm"][1]).max())
    assert l / q > 1e5, (q, l)
    # silent channels: the scale is 0 (both blocks zero) on some emitted packets, and the model's output there is exactly 0
    ms = sm.model_of(spec, pr["silent"])
    zero = (ms["scale"] == 0) & (ms["emit_len"][:, None] > 0)
    assert zero.sum() > 10


def test_model_frame_counts_streaming_across_submits():
    """One stream cut into submits (model handle and oracle handle continuing alike) == the uncut stream, frames and PCM."""
    spec = fixture_like_spec(2)
    b = synth_batch(spec, 1, 60, "mixed", seed=3, unused_frac=0.2, granule_last=True)
    whole = sm.SynthModel(spec, 1).submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"])
    n = np.where(b["packets"]["mode"] == 1, spec.blocksize1, spec.blocksize0)
    off = np.concatenate([[0], np.cumsum(n // 2 * spec.channels)])
    m, o = sm.SynthModel(spec, 2), ob.OracleSynth(spec, 2)
    parts = []
    cuts = [0, 1, 2, 13, 14, 40, 60]
    for a, e in zip(cuts[:-1], cuts[1:]):
        seg = b["segments"].copy()
        seg["stream"], seg["first_packet"], seg["num_packets"], seg["flags"], seg["residue_off"] = 1, 0, e - a, 1 if a == 0 else 0, 0
        args = (b["packets"][a:e], seg, b["ys"][a:e], b["residue"][off[a]:off[e]], b["plane_stride"])
        r, w = m.submit_host(*args), o.submit_host(*args)
        assert np.array_equal(r["emit_len"], w["emit_len"])
        assert np.array_equal(r["emit_len"], whole["emit_len"][a:e])
        assert np.array_equal(r["scale"], whole["scale"][a:e])
        sm.gate(w["pcm"], r, seg)
        parts.append(r["pcm"][0][:, :int(r["emit_len"].sum())])
    total = int(whole["emit_len"].sum())
    assert np.array_equal(np.concatenate(parts, axis=1), whole["pcm"][0][:, :total])


def test_model_frame_counts_granules_and_resets():
    """Clipped last packets (granule_last), a stream slot reused with VSYN_SEG_RESET in a later submit, empty segments."""
    spec = fixture_like_spec(1, 128, 1024)
    m, o = sm.SynthModel(spec, 3), ob.OracleSynth(spec, 3)
    for seed in (1, 2):
        b = synth_batch(spec, 3, 17 + seed, "mixed", seed=seed, granule_last=True, unused_frac=0.5)
        r = m.submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"])
        w = o.submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"])
        assert np.array_equal(r["emit_len"], w["emit_len"])
        sm.gate(w["pcm"], r, b["segments"])
    seg = np.zeros(1, b["segments"].dtype)
    seg["stream"] = 2
    r = m.submit_host(b["packets"][:0], seg, b["ys"][:0], b["residue"][:0], 8)
    assert r["pcm"].shape == (1, 1, 8) and not r["pcm"].any()


def test_disagreeing_window_flags_are_outside_the_model():
    spec = fixture_like_spec(2)
    b = synth_batch(spec, 1, 12, "mixed", seed=4)
    b["packets"]["next_long"][0] = 0  # long block in front of a long one, next_long clear (class C)
    with pytest.raises(AssertionError):
        sm.SynthModel(spec, 1).submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"])


@pytest.mark.parametrize("name", ["test.stereo44khz", "test.mono44khz"])
def test_reference_fixtures_in_gate(name):
    """The reference's own hooks on its .ogg fixtures: its 'pcm' hook and the oracle both within G of the model."""
    spec, b, z = load_golden(name)
    total = b["pcm"].shape[1]
    bb = dict(b, plane_stride=total + 8)
    m = sm.model_of(spec, bb)
    assert np.array_equal(m["emit_len"], b["emit_len"])
    ref = np.zeros((1, spec.channels, total + 8), np.float32)
    ref[0, :, :total] = b["pcm"]
    r = sm.per_packet_error(ref, m, b["segments"])
    _note(r, m["n"])
    sm.gate(ref, m, b["segments"], ctx="reference pcm hook")
    _oracle_in_gate(spec, bb, ctx=name)
    print("%s: reference pcm hook worst %.1f x 2^-24 s" % (name, r.max()))


def _synth_names():
    return ["synth_%02d" % i for i in range(20)]


@pytest.mark.parametrize("name", _synth_names())
def test_synthetic_stream_fixtures_in_gate(name, tmp_path_factory):
    """The 20 synth_NN streams (synth_16 / 17: floors whose x[1] is not half the block size; synth_18 / 19: a floor per (mapping, submap)
    and several modes per block size), fed as test_oracle_golden feeds them (fixture setup + the host entropy probe)."""
    from tests.test_oracle_golden import _oracle_on_stream
    from tests.workloads import fixture_setup
    res, z, d = _oracle_on_stream(name, tmp_path_factory)
    assert res["rc"] == 0
    spec = fixture_setup(name)
    seg = np.zeros(1, dtype=res_seg_dtype())
    seg["num_packets"], seg["flags"] = d["P"], 1
    b = dict(packets=d["packets"], segments=seg, ys=d["ys"], residue=d["residue"], plane_stride=res["pcm"].shape[2])
    if not sm.agreeing_flags(spec, b["packets"], seg):
        pytest.fail("synthetic stream fixture %s has window flags that disagree with its blocks" % name)
    m = sm.model_of(spec, b)
    assert np.array_equal(m["emit_len"], res["emit_len"])
    r = sm.per_packet_error(res["pcm"], m, seg)
    _note(r, m["n"])
    sm.gate(res["pcm"], m, seg, ctx=name)


def res_seg_dtype():
    from parseoggvorbis_amd.binding import SEGMENT_DTYPE
    return SEGMENT_DTYPE


def _digest(b):
    h = hashlib.sha256()
    for k in ("packets", "segments", "ys", "residue"):
        h.update(np.ascontiguousarray(b[k]).tobytes())
    h.update(str(int(b["plane_stride"])).encode())
    return h.hexdigest()


def test_synth_batch_defaults_unchanged():
    """Digests taken before the residue kinds, residue scale, per-stream floor ranges and alternating loudness were added."""
    cases = [((2, 256, 2048), dict(streams=3, packets_per_stream=40, pattern="mixed", seed=7),
              "85b9cf3eefc62c35223436b9e8d19b6e0f3c2b435ae71213a917f58f9d94bc69"),
             ((1, 64, 8192), dict(streams=2, packets_per_stream=14, pattern="mixed", seed=1, unused_frac=0.1, granule_last=True),
              "e55bbd7b7a00b7e8886aa743bf90b2e26f4ced8f2d0a95d2e5b929e3e6f84646"),
             ((3, 128, 1024), dict(streams=2, packets_per_stream=21, pattern="long", seed=5, unused_frac=0.3),
              "5f06374bad8b5a4563fcd5804092409e7cda7c334f65635cf58bee09500317dd"),
             ((2, 512, 4096), dict(streams=1, packets_per_stream=9, pattern=[1, 0, 0, 1, 1, 0, 1, 1, 0], seed=9, ylo=10, yhi=30),
              "3a1af37aeab8b1dcb84cf6be9ad4f3c86a8fab8d20abfec97013b3b8a653218f")]
    for (C, bs0, bs1), kw, want in cases:
        assert _digest(synth_batch(fixture_like_spec(C, bs0, bs1), **kw)) == want, (C, bs0, bs1, kw)


def test_zz_print_the_oracles_worst_ratio_per_block_size():
    """Runs last in this module: the oracle's largest max|d| / (2^-24 s) per block size over the cases above, all under G."""
    print("oracle worst max|d| / (2^-24 s) per block size: %s (gate %g)" % ({k: round(v, 1) for k, v in sorted(WORST.items())}, sm.G))
    assert all(v <= sm.G for v in WORST.values())
