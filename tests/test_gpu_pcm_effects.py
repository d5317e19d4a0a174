"""PCM effects on the GPU (include/vorbis_synth_hip.h, "PCM effects": vsyn_pcm_hpss_device, vsyn_pcm_chain_effects_host,
ogg_vorbis_pcm_corpus_effects, get_pcm_batch(mono=True, hpss=...)).

The stage is a composition of stages that have tests of their own, so everything below the end-to-end test compares bytes: the stage
against the same composition through the public device entry points (vsyn_spectral_device lin_power / 1, vsyn_spectral_hpss_device
with the mask output, vsyn_spectral_device stft, vsyn_istft_device under that mask), and the stages behind it against those stages
run on its output. The end-to-end test uses the bounds of tests/spectral_lin_model.py and tests/istft_model.py."""
import os

import numpy as np
import pytest

from tests import istft_model as im
from tests import spectral_lin_model as lm
from tests import loudness_model as ldm
from tests import spectral_model as sm
from tests.test_gpu_loudness import _cond_device, _run_stage, _same_records, _spec as _loud_spec

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _effect(component="harmonic", n_fft=1024, hop=256, win=None, kernel=31, power=2.0, margin=1.0):
    from parseoggvorbis_amd.binding import PcmEffect, SpectralHpss
    return PcmEffect(n_fft, hop, n_fft if win is None else win, 0,
                     SpectralHpss(kernel, kernel, 1 if component == "percussive" else 0, 0, power, margin, margin))


def compose(g, eff, segs):
    """The effect through the public device entries on segs (a list of (C, T) float32): (the components, a list of float32 [T];
    the masks, a list of float32 [F][NB])."""
    import torch
    from parseoggvorbis_amd import spectral
    from parseoggvorbis_amd.binding import SpectralHpss
    S, Cn = len(segs), segs[0].shape[0]
    T = [s.shape[1] for s in segs]
    plane = max(T + [1])
    n, hop, win = eff.n_fft, eff.hop_length, eff.win_length
    nb = n // 2 + 1
    pcm = np.zeros((S, Cn, plane), np.float32)
    for i, s in enumerate(segs):
        pcm[i, :, :T[i]] = s
    rows = [sm.num_frames(t, n, hop, True) for t in T]
    total = sum(rows)
    stream = torch.cuda.current_stream().cuda_stream
    d_pcm = torch.from_numpy(pcm).cuda()
    d_frames = torch.from_numpy(np.asarray(T, np.int32)).cuda()
    d_mag = torch.zeros((total + 1, nb), dtype=torch.float32, device="cuda")
    d_mask = torch.zeros((total + 1, nb), dtype=torch.float32, device="cuda")
    d_stft = torch.zeros((total + 1, 2 * nb), dtype=torch.float32, device="cuda")
    d_out = torch.zeros((S, plane), dtype=torch.float32, device="cuda")
    mag = spectral.spectral_spec("lin_power", n_fft=n, hop_length=hop, win_length=win, center=True, power=1)
    fwd = spectral.spectral_spec("stft", n_fft=n, hop_length=hop, win_length=win, center=True)
    hp = eff.hpss
    mask = SpectralHpss(hp.kh, hp.kp, hp.component, 1, hp.power, hp.margin_h, hp.margin_p)
    g.spectral_device(mag, [1] * S, d_pcm.data_ptr(), plane, Cn, d_frames.data_ptr(), d_mag.data_ptr(), None, stream)
    g.spectral_hpss_device(mask, nb, rows, d_mag.data_ptr(), d_mask.data_ptr(), stream)
    g.spectral_device(fwd, [1] * S, d_pcm.data_ptr(), plane, Cn, d_frames.data_ptr(), d_stft.data_ptr(), None, stream)
    g.istft_device(fwd, rows, d_stft.data_ptr(), d_mask.data_ptr(), T, d_out.data_ptr(), plane, None, stream)
    torch.cuda.synchronize()
    out, m = d_out.cpu().numpy(), d_mask.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(rows)])
    return [out[i, :T[i]].copy() for i in range(S)], [m[off[i]:off[i + 1]] for i in range(S)]


def stage_alone(g, eff, segs):
    """vsyn_pcm_hpss_device on segs: a list of float32 [T]; NaN sentinels behind every segment's frames must stay."""
    import torch
    S, Cn = len(segs), segs[0].shape[0]
    T = [s.shape[1] for s in segs]
    plane = max(T + [1]) + 3
    pcm = np.full((S, Cn, plane), np.nan, np.float32)
    for i, s in enumerate(segs):
        pcm[i, :, :T[i]] = s
    d_pcm = torch.from_numpy(pcm).cuda()
    d_out = torch.full((S, plane + 2), float("nan"), dtype=torch.float32, device="cuda")
    d_fr = torch.zeros(S, dtype=torch.int32, device="cuda")
    g.pcm_hpss_device(eff, T, d_pcm.data_ptr(), plane, Cn, d_out.data_ptr(), plane + 2, d_fr.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert list(d_fr.cpu().numpy()) == T
    assert all(np.isnan(out[i, T[i]:]).all() for i in range(S))
    assert np.array_equal(d_pcm.cpu().numpy().view(np.uint32), pcm.view(np.uint32))
    return [out[i, :T[i]].copy() for i in range(S)]


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_chain():
    """effect = NULL is vsyn_pcm_chain_host; with an effect the PCM is the composition through the public device entries, bit for
    bit, ungated on the stereo planes and behind a trim and a split on the mono plane, at two framings and both components; loudness
    and conditioning behind it equal those stages run on its output; refusals write nothing; vsyn_pcm_fetch_host and the next
    submit are unchanged around all of it."""
    from parseoggvorbis_amd import binding
    from parseoggvorbis_amd.binding import PcmCond, PcmTrim, Synth, VsynError, VSYN_PCM_F32, VSYN_PCM_S16
    from tests.workloads import fixture_like_spec, synth_batch
    spec = fixture_like_spec(2)
    b1 = synth_batch(spec, streams=3, packets_per_stream=64, pattern="mixed", seed=11)
    b2 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=12)
    S = len(b1["segments"])
    rates = [16000, 8000, 12000][:S]
    gp = Synth(spec, device=0, max_streams=4)
    planar = gp.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"])["pcm"]
    gp.close()
    trim, pre, loud = PcmTrim(256, 64, 40.0), PcmCond(2, 0, 0.97), _loud_spec(mono=True)
    outs = []
    for with_effect in (False, True):
        g = Synth(spec, device=0, max_streams=4)
        assert g.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"], flags=4)["rc"] == 0  # KEEP_PCM
        f1, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        if with_effect:
            _, frames, _ = g.pcm_condition_host(PcmCond(0, 0, 0.0), S)
            stereo = [planar[s][:, :int(frames[s])] for s in range(S)]
            assert min(x.shape[1] for x in stereo) > 4096
            # effect = NULL: the entry without the argument
            for gate, split, ld, cd in ((trim, False, None, pre), (trim, True, loud, None), (None, False, loud, pre)):
                a = g.pcm_chain_effects_host(gate, split, None, ld, cd, S, rates)
                b = g.pcm_chain_host(gate, split, ld, cd, S, rates)
                assert _bits(a["pcm"], b["pcm"]) and np.array_equal(a["frames"], b["frames"]) and _same_records(a["records"], b["records"])
                assert np.array_equal(a["peaks"], b["peaks"]) and np.array_equal(a["refs"], b["refs"]) and np.array_equal(a["bounds"], b["bounds"])
            for eff in (_effect("harmonic", 1024, 256), _effect("percussive", 64, 16, 48, kernel=(7), power=1.0, margin=2.0)):
                # ungated: the stage reads the stereo planes and downmixes as the spectral stage does
                want, _ = compose(g, eff, stereo)
                alone = stage_alone(g, eff, stereo)
                on = g.pcm_chain_effects_host(None, False, eff, None, None, S, rates)
                assert np.array_equal(on["frames"], frames)
                for s in range(S):
                    T = int(frames[s])
                    assert want[s].any() and _bits(alone[s], want[s]), (s, eff.n_fft)
                    assert _bits(on["pcm"][s][:T], want[s]) and not on["pcm"][s][T:].any(), (s, eff.n_fft)
                # behind a gate: the stage reads the gate's mono plane with the gate's frames
                for split in (False, True):
                    plain = g.pcm_chain_host(trim, split, None, None, S, rates)
                    mono = [plain["pcm"][s][None, :int(plain["frames"][s])] for s in range(S)]
                    want, _ = compose(g, eff, mono)
                    on = g.pcm_chain_effects_host(trim, split, eff, None, None, S, rates)
                    assert np.array_equal(on["frames"], plain["frames"]) and np.array_equal(on["refs"], plain["refs"])
                    assert np.array_equal(on["counts"], plain["counts"]) if split else np.array_equal(on["bounds"], plain["bounds"])
                    for s in range(S):
                        T = int(plain["frames"][s])
                        assert _bits(on["pcm"][s][:T], want[s]) and not on["pcm"][s][T:].any(), (split, s)
                # the stages behind it act on the component: loudness, then conditioning
                for gate in (None, trim):
                    on = g.pcm_chain_effects_host(gate, False, eff, None, None, S, rates)
                    segs = [on["pcm"][s][None, :int(on["frames"][s])] for s in range(S)]
                    lalone = _run_stage(g, _loud_spec(), segs, rates, outputs=True)
                    with_loud = g.pcm_chain_effects_host(gate, False, eff, loud, None, S, rates)
                    assert _same_records(with_loud["records"], lalone["rec"]) and (with_loud["records"]["status"] == ldm.OK).any()
                    for s in range(S):
                        T = int(on["frames"][s])
                        assert _bits(with_loud["pcm"][s][:T], lalone["scaled"][s][0]) and not with_loud["pcm"][s][T:].any()
                    both = g.pcm_chain_effects_host(gate, False, eff, loud, pre, S, rates)
                    assert _bits(both["pcm"], _cond_device(g, pre, with_loud["pcm"], with_loud["frames"]))
                    peak = g.pcm_chain_effects_host(gate, False, eff, None, PcmCond(3, 0, 0.97), S, rates)
                    assert _bits(peak["pcm"], _cond_device(g, PcmCond(3, 0, 0.97), on["pcm"], on["frames"]))
                # resampled first, and int16 out: the component of the resampled signal, converted as every int16 output is
                rs, rs_frames = g.pcm_resample_host(rates, 16000)
                want, _ = compose(g, eff, [rs[s][:, :int(rs_frames[s])] for s in range(S)])
                on = g.pcm_chain_effects_host(None, False, eff, None, None, S, rates, 16000)
                s16 = g.pcm_chain_effects_host(None, False, eff, None, None, S, rates, 16000, VSYN_PCM_S16)
                for s in range(S):
                    T = int(rs_frames[s])
                    assert _bits(on["pcm"][s][:T], want[s])
                    assert s16["pcm"].dtype == np.int16 and not s16["pcm"][s][T:].any()
                    assert np.abs(s16["pcm"][s][:T] - np.clip(want[s].astype(np.float64) * 32768.0, -32768, 32767)).max() <= 1.0
            # refusals: nothing is written
            for bad in (_effect(n_fft=1000, hop=250), _effect(n_fft=8, hop=2), _effect(n_fft=16384, hop=4096), _effect(hop=0), _effect(win=2048),
                        _effect(kernel=30), _effect(margin=0.5), _effect(power=0.0)):
                out, fr = np.full((S, 8), 7.0, np.float32), np.full(S, 7, np.uint64)
                err = binding.C.c_char_p()
                rc = g.lib.vsyn_pcm_chain_effects_host(g.h, None, 0, binding.C.byref(bad), None, None, S, binding._ptr(binding._rates(rates)), 0,
                                                       VSYN_PCM_F32, binding._ptr(out), 8, binding._ptr(fr), None, None, None, 0, None, None, None,
                                                       binding.C.byref(err))
                assert rc == binding.VSYN_ERR_INVALID and (out == 7.0).all() and (fr == 7).all(), err.value
            for output in (1, 2):
                bad = _effect()
                bad.hpss.output = output
                with pytest.raises(VsynError) as ei:
                    g.pcm_chain_effects_host(None, False, bad, None, None, S, rates)
                assert ei.value.code == binding.VSYN_ERR_INVALID and "component" in str(ei.value)
            with pytest.raises(VsynError) as ei:
                g.pcm_chain_effects_host(None, False, _effect(n_fft=1000, hop=250), None, None, S, rates)
            assert "power of two" in str(ei.value)
        f1b, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        assert np.array_equal(f1, f1b)
        r2 = g.submit_host(b2["packets"], b2["segments"], b2["ys"], b2["residue"], b2["plane_stride"])
        assert r2["rc"] == 0
        outs.append((f1, r2["pcm"], r2["emit_len"]))
        g.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])


@pytest.fixture(scope="module")
def stereo_ogg():
    with open(os.path.join(GOLDEN, "test.stereo44khz.ogg"), "rb") as f:
        return f.read()


def test_end_to_end(stereo_ogg):
    """get_pcm_batch(mono=True, hpss=...) on the stereo fixture, compared over its first two seconds. The masks of the two
    components at margin 1 sum to 1, "bad" elements included. The harmonic and the percussive component sum to the plain mono PCM
    within the two inverse bounds and twice the forward bound: both are inverses of the same device X (within B_f of the model's per
    component, which the masked inverse carries as at most 2 B_f per sample of a frame, the masks being at most 1) under masks whose
    sum is within 2 u of 1, which the mask term u A_f of each inverse bound covers; the model inverse of the model X is the float64
    mean of the channels, from which the float32 mono PCM is (C + 1) u mean |x_c| away. float32 and int16; behind a trim; a damaged
    file fails alone."""
    from parseoggvorbis_amd import pcm
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec
    n, hop = 1024, 256
    kw = dict(mono=True, hpss_n_fft=n, hpss_hop_length=hop)
    planes, sr = pcm.get_pcm_batch([stereo_ogg])[0]
    plain = pcm.get_pcm_batch([stereo_ogg], mono=True)[0][0]
    har, sr_h = pcm.get_pcm_batch([stereo_ogg], hpss="harmonic", **kw)[0]
    per, sr_p = pcm.get_pcm_batch([stereo_ogg], hpss="percussive", **kw)[0]
    assert sr == sr_h == sr_p == 44100 and plain.dtype == har.dtype == per.dtype == np.float32 and planes.shape[0] == 2
    L = plain.shape[0]
    assert plain.shape == har.shape == per.shape == (L,) and L > 8 * n
    assert har.any() and per.any() and not np.array_equal(har, per)
    # The model runs on a cut: sample t < T lies under frames that start below T + n / 2, whose masks read 15 frames further, and
    # those frames read n / 2 samples further still; none of them must see the cut or be reflected at it.
    T = min(L, 2 * 44100)
    Tm = T + n + 20 * hop
    if Tm >= L:
        T = Tm = L
    x = planes[:, :Tm]
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    try:
        ch, mh = compose(g, _effect("harmonic", n, hop), [x])
        cp, mp = compose(g, _effect("percussive", n, hop), [x])
    finally:
        g.close()
    assert np.abs(mh[0].astype(np.float64) + mp[0].astype(np.float64) - 1.0).max() <= 2.0 ** -23  # two roundings of values in [0, 1]
    assert _bits(har[:T], ch[0][:T]) and _bits(per[:T], cp[0][:T])  # the file's components are the composition's
    X, B = lm.stft(x, n, hop, n, True)
    w = lm.window32(n, n).astype(np.float64)
    carried = im.overlap_add(np.zeros((X.shape[0], n)), w, n, hop, n, True, Tm, dv=w[None, :] * 2.0 * B[:, None])[3]
    bh = im.istft(X, n, hop, n, True, Tm, mask=mh[0])[1]
    bp = im.istft(X, n, hop, n, True, Tm, mask=mp[0])[1]
    mean = x.astype(np.float64).mean(axis=0)
    assert np.abs(im.istft(X, n, hop, n, True, Tm)[0] - mean)[:T].max() < 1e-12
    tol = ((bh + bp) * 1.001 + 2.0 * carried + 4.0 * lm.U * np.abs(x.astype(np.float64)).mean(axis=0))[:T]
    d = np.abs(har[:T].astype(np.float64) + per[:T].astype(np.float64) - plain[:T].astype(np.float64))
    print("harmonic + percussive - mono: worst |d| / bound %.2e (|d| max %.3g)" % (float((d / tol).max()), float(d.max())))
    assert (d <= tol).all()
    # int16: the conversion of the float32 component that every int16 output has
    h16, _ = pcm.get_pcm_batch([stereo_ogg], dtype="int16", hpss="harmonic", **kw)[0]
    assert h16.dtype == np.int16 and h16.shape == har.shape
    assert np.abs(h16.astype(np.float64) - np.clip(har.astype(np.float64) * 32768.0, -32768, 32767)).max() <= 1.0
    # behind a trim the component is that of what is kept, and hpss=None is the call without the argument
    idx = []
    cut, _ = pcm.get_pcm_batch([stereo_ogg], trim_db=20.0, trim_index=idx, hpss="harmonic", **kw)[0]
    assert cut.shape[0] == idx[0][1] - idx[0][0] and cut.any()
    assert np.array_equal(pcm.get_pcm_batch([stereo_ogg], mono=True, hpss=None, hpss_n_fft=3)[0][0], plain)
    # a damaged file fails alone
    bad = bytearray(stereo_ogg)
    bad[len(bad) // 2] ^= 0x55  # a page CRC
    res = pcm.get_pcm_batch([stereo_ogg, bytes(bad), stereo_ogg], errors="return", files_per_submit=2, hpss="percussive", **kw)
    assert isinstance(res[1], pcm.PcmError) and "file 1" in str(res[1])
    assert np.array_equal(res[0][0], per) and np.array_equal(res[2][0], per)
    with pytest.raises(pcm.PcmError):
        pcm.get_pcm_batch([stereo_ogg, bytes(bad)], hpss="percussive", **kw)
