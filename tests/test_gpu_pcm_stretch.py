"""PCM stretch on the GPU (include/vorbis_synth_hip.h, "PCM stretch": vsyn_pcm_stretch_device, vsyn_pcm_chain_stretch_host,
ogg_vorbis_pcm_corpus_stretch, get_pcm_batch(mono=True, time_stretch= / pitch_shift=)).

The stage is a composition of stages that have tests of their own (the phase vocoder's: tests/test_gpu_pv.py), so everything here
compares bytes: the stage against the same composition through the public device entry points (vsyn_spectral_device stft,
vsyn_phase_vocoder_device, vsyn_istft_device to vsyn_stretch_num_samples, vsyn_resample_device, the length fix), and the stages
around it in a chain against those stages run on its input and output."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import pv_model as pm
from tests import spectral_model as sm
from tests.test_gpu_loudness import TARGET, _cond_device, _run_stage, _same_records, _spec as _loud_spec

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RATES = [0.8, 1.0, 1.25, 2.0 ** (3.0 / 12.0)]
GUARD = 3


def _stretch(n_fft=1024, hop=256, win=None, fix=False, to_hz=0):
    from parseoggvorbis_amd.binding import PcmStretch
    return PcmStretch(n_fft, hop, n_fft if win is None else win, 1 if fix else 0, to_hz, 0)


def _from_hz(sr, rates):
    return [int(np.rint(sr / r)) for r in rates]


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def synth():
    import torch
    assert torch.cuda.is_available()
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    yield g
    g.close()


def compose(g, st, segs, rates, from_hz=None):
    """The stage through the public device entries on segs (a list of (C, T) float32): a list of float32 [delivered frames]."""
    import torch
    from parseoggvorbis_amd import spectral
    S, Cn = len(segs), segs[0].shape[0]
    T = [s.shape[1] for s in segs]
    plane = max(T + [1])
    n, hop, win = st.n_fft, st.hop_length, st.win_length
    nb = n // 2 + 1
    pcm = np.zeros((S, Cn, plane), np.float32)
    for i, s in enumerate(segs):
        pcm[i, :, :T[i]] = s
    rows = [sm.num_frames(t, n, hop, True) for t in T]
    rows_out = [g.lib.vsyn_pv_num_rows(f, float(r)) for f, r in zip(rows, rates)]
    L = [g.lib.vsyn_stretch_num_samples(t, float(r)) for t, r in zip(T, rates)]
    assert L == [pm.num_samples(t, r) for t, r in zip(T, rates)]
    stream = torch.cuda.current_stream().cuda_stream
    d_pcm = torch.from_numpy(pcm).cuda()
    d_frames = torch.from_numpy(np.asarray(T, np.int32)).cuda()
    d_stft = torch.zeros((sum(rows) + 1, 2 * nb), dtype=torch.float32, device="cuda")
    d_pv = torch.zeros((sum(rows_out) + 1, 2 * nb), dtype=torch.float32, device="cuda")
    lplane = max(L + [1])
    d_out = torch.zeros((S, lplane), dtype=torch.float32, device="cuda")
    d_len = torch.zeros(S, dtype=torch.int32, device="cuda")
    fwd = spectral.spectral_spec("stft", n_fft=n, hop_length=hop, win_length=win, center=True)
    g.spectral_device(fwd, [1] * S, d_pcm.data_ptr(), plane, Cn, d_frames.data_ptr(), d_stft.data_ptr(), None, stream)
    assert list(g.phase_vocoder_device(fwd, rows, rates, d_stft.data_ptr(), d_pv.data_ptr(), stream)) == rows_out
    g.istft_device(fwd, rows_out, d_pv.data_ptr(), None, L, d_out.data_ptr(), lplane, d_len.data_ptr(), stream)
    n_out = L
    if st.shift_to_hz:
        n_out = [g.lib.vsyn_resample_num_frames(f, st.shift_to_hz, l) for f, l in zip(from_hz, L)]
        rplane = max([g.lib.vsyn_resample_num_frames(f, st.shift_to_hz, lplane) for f in from_hz] + [1])  # what the entry asks of the stride
        d_rs = torch.zeros((S, rplane), dtype=torch.float32, device="cuda")
        d_rf = torch.zeros(S, dtype=torch.int32, device="cuda")
        g.resample_device(from_hz, st.shift_to_hz, d_out.data_ptr(), lplane, 1, d_len.data_ptr(), d_rs.data_ptr(), rplane, d_rf.data_ptr(), stream)
        d_out = d_rs
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    res = []
    for i in range(S):
        y = out[i, :n_out[i]]
        if st.options & 1:  # the length fix: cut, or followed by zeros
            z = np.zeros(T[i], np.float32)
            z[:min(T[i], len(y))] = y[:T[i]]
            y = z
        res.append(y.copy())
    return res


def stage_alone(g, st, segs, rates, from_hz=None, slack=GUARD):
    """vsyn_pcm_stretch_device on segs: a list of float32 [delivered frames]; the NaN guard words behind every segment's frames and
    behind out_plane_stride must stay, the input unchanged, d_out_frames the delivered frames."""
    import torch
    S, Cn = len(segs), segs[0].shape[0]
    T = [s.shape[1] for s in segs]
    plane = max(T + [1]) + 3
    pcm = np.full((S, Cn, plane), np.nan, np.float32)
    for i, s in enumerate(segs):
        pcm[i, :, :T[i]] = s
    L = [pm.num_samples(t, r) for t, r in zip(T, rates)]
    if st.options & 1:
        want = T
    elif st.shift_to_hz:
        want = [g.lib.vsyn_resample_num_frames(f, st.shift_to_hz, l) for f, l in zip(from_hz, L)]
    else:
        want = L
    oplane = max(want + [1]) + slack
    d_pcm = torch.from_numpy(pcm).cuda()
    d_out = torch.full((S * oplane + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    d_fr = torch.full((S + 1,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    g.pcm_stretch_device(st, T, rates, from_hz, d_pcm.data_ptr(), plane, Cn, d_out.data_ptr(), oplane, d_fr.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    flat = d_out.cpu().numpy()
    out, fr = flat[:S * oplane].reshape(S, oplane), d_fr.cpu().numpy()
    assert list(fr[:S]) == want and fr[S] == 0x7FFFFFFF
    assert np.isnan(flat[S * oplane:]).all() and all(np.isnan(out[i, want[i]:]).all() for i in range(S)), "guard words"
    assert np.array_equal(d_pcm.cpu().numpy().view(np.uint32), pcm.view(np.uint32))
    return [out[i, :want[i]].copy() for i in range(S)]


@pytest.mark.parametrize("n,hop", [(64, 16), (1024, 256)])
def test_stage_equals_the_composition(synth, n, hop):
    """Stereo planes of 0, 1, 100 and 3000 frames, each at every rate (the rates rotate through the segments over four calls): the
    stretch alone, with the length fixed, and with a shift back to 8000 Hz with and without the fix; a plane stride with no slack."""
    rng = np.random.default_rng(n)
    frames = [0, 1, 100, 3000]
    segs = [(0.25 * rng.standard_normal((2, t))).astype(np.float32) for t in frames]
    sr = 8000
    for rot in range(4):
        rates = RATES[rot:] + RATES[:rot]
        hz = _from_hz(sr, rates)
        for st, fh in ((_stretch(n, hop), None), (_stretch(n, hop, fix=True), None), (_stretch(n, hop, to_hz=sr), hz),
                       (_stretch(n, hop, n - 7, fix=True, to_hz=sr), hz)):
            want = compose(synth, st, segs, rates, fh)
            got = stage_alone(synth, st, segs, rates, fh, slack=GUARD if rot else 0)
            for s, t in enumerate(frames):
                assert _bits(got[s], want[s]), (n, rot, st.options, st.shift_to_hz, s)
                if st.options & 1:
                    assert len(got[s]) == t
                    have = pm.num_samples(t, rates[s])
                    if st.shift_to_hz:
                        have = synth.lib.vsyn_resample_num_frames(hz[s], sr, have)
                    assert not got[s][have:].any()  # the zeros behind what the stage made
                elif not st.shift_to_hz:
                    assert len(got[s]) == int(round(t / rates[s]))
            assert got[3].any() and np.isfinite(got[3]).all()


def test_stage_refusals_leave_the_outputs_untouched(synth):
    import torch
    n, hop, T = 64, 16, 100
    d_pcm = torch.ones((1, 1, T), dtype=torch.float32, device="cuda")
    d_out = torch.full((2 * T,), float("nan"), dtype=torch.float32, device="cuda")
    d_fr = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    lib, err = synth.lib, C.c_char_p()
    fr = np.array([T], np.uint64)

    def call(st, rate=1.0, hz=None, plane=2 * T):
        r = np.array([rate], np.float64)
        h = None if hz is None else np.array([hz], np.uint32)
        rc = lib.vsyn_pcm_stretch_device(synth.h, C.byref(st), 1, C.c_void_p(fr.ctypes.data), C.c_void_p(r.ctypes.data),
                                         None if h is None else C.c_void_p(h.ctypes.data), d_pcm.data_ptr(), T, 1, d_out.data_ptr(), plane,
                                         d_fr.data_ptr(), stream, C.byref(err))
        return rc, (err.value or b"").decode()

    bad_opt, bad_res = _stretch(n, hop), _stretch(n, hop)
    bad_opt.options, bad_res.reserved = 2, 1
    for word, kw in [("power of two", dict(st=_stretch(1000, 250))), ("n_fft", dict(st=_stretch(8, 2))), ("hop_length", dict(st=_stretch(n, 0))),
                     ("win_length", dict(st=_stretch(n, hop, n + 1))), ("options", dict(st=bad_opt)), ("reserved", dict(st=bad_res)),
                     ("rate", dict(st=_stretch(n, hop), rate=0.0)), ("rate", dict(st=_stretch(n, hop), rate=float("nan"))),
                     ("rate", dict(st=_stretch(n, hop), rate=float("inf"))), ("shift_from_hz", dict(st=_stretch(n, hop, to_hz=8000))),
                     ("shift_from_hz", dict(st=_stretch(n, hop, to_hz=8000), hz=0)),
                     ("above the limit", dict(st=_stretch(n, hop, to_hz=65537), hz=65539)),  # the resampler's refusal, by name
                     ("out_plane_stride", dict(st=_stretch(n, hop), rate=0.5, plane=2 * T - 1)),
                     ("out_plane_stride", dict(st=_stretch(n, hop, fix=True), rate=2.0, plane=T - 1))]:
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (word, rc, msg)
    torch.cuda.synchronize()
    assert np.isnan(d_out.cpu().numpy()).all() and int(d_fr.cpu()[0]) == 77
    rc, msg = call(_stretch(n, hop), rate=0.5)  # and a call with nothing wrong runs, into a plane with no slack
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert np.isfinite(d_out.cpu().numpy()).all() and int(d_fr.cpu()[0]) == 2 * T


def test_chain_on_a_submit():
    """stretch = NULL is vsyn_pcm_chain_effects_host, bit for bit; with a stretch frames_out is the stretched count, the PCM the
    stage's on the plane the chain has there (ungated: the stereo planes; gated: the gate's mono plane), the loudness and conditioning
    steps take the stage's frames; an out_stride_frames one below the need, and a stretch beside an effect, are refused with the
    outputs untouched; vsyn_pcm_fetch_host is unchanged around all of it."""
    from parseoggvorbis_amd import binding
    from parseoggvorbis_amd.binding import PcmCond, PcmTrim, Synth, VsynError, VSYN_PCM_F32
    from tests.test_gpu_pcm_effects import _effect
    from tests.workloads import fixture_like_spec, synth_batch
    spec = fixture_like_spec(2)
    b1 = synth_batch(spec, streams=3, packets_per_stream=64, pattern="mixed", seed=11)
    S = len(b1["segments"])
    rates = [16000, 8000, 12000][:S]
    trim, pre, loud = PcmTrim(256, 64, 40.0), PcmCond(2, 0, 0.97), _loud_spec(mono=True)
    gp = Synth(spec, device=0, max_streams=4)
    planar = gp.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"])["pcm"]
    gp.close()
    g = Synth(spec, device=0, max_streams=4)
    try:
        assert g.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"], flags=4)["rc"] == 0  # KEEP_PCM
        f1, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        _, frames, _ = g.pcm_condition_host(PcmCond(0, 0, 0.0), S)
        stereo = [planar[s][:, :int(frames[s])] for s in range(S)]
        for gate, split, eff, ld, cd in ((trim, False, None, None, pre), (trim, True, _effect("harmonic", 64, 16), loud, None),
                                         (None, False, None, loud, pre)):
            a = g.pcm_chain_stretch_host(gate, split, eff, None, None, None, ld, cd, S, rates)
            b = g.pcm_chain_effects_host(gate, split, eff, ld, cd, S, rates)
            assert _bits(a["pcm"], b["pcm"]) and np.array_equal(a["frames"], b["frames"]) and _same_records(a["records"], b["records"])
            assert np.array_equal(a["peaks"], b["peaks"]) and np.array_equal(a["refs"], b["refs"]) and np.array_equal(a["bounds"], b["bounds"])
        sr_rates = [0.8, 1.25, 2.0 ** (3.0 / 12.0)][:S]
        for st, hz in ((_stretch(1024, 256), None), (_stretch(64, 16, 48, fix=True, to_hz=8000), _from_hz(8000, sr_rates))):
            want = compose(g, st, stereo, sr_rates, hz)
            on = g.pcm_chain_stretch_host(None, False, None, st, sr_rates, hz, None, None, S, rates)
            assert list(on["frames"]) == [len(w) for w in want]
            if not st.options:
                assert list(on["frames"]) == [int(round(int(t) / r)) for t, r in zip(frames, sr_rates)]
            for s in range(S):
                T = len(want[s])
                assert want[s].any() and _bits(on["pcm"][s][:T], want[s]) and not on["pcm"][s][T:].any(), (s, st.n_fft)
            for split in (False, True):  # behind a gate: the stage reads the gate's mono plane with the gate's frames
                plain = g.pcm_chain_host(trim, split, None, None, S, rates)
                mono = [plain["pcm"][s][None, :int(plain["frames"][s])] for s in range(S)]
                want = compose(g, st, mono, sr_rates, hz)
                on = g.pcm_chain_stretch_host(trim, split, None, st, sr_rates, hz, None, None, S, rates)
                assert list(on["frames"]) == [len(w) for w in want] and np.array_equal(on["refs"], plain["refs"])
                assert np.array_equal(on["counts"], plain["counts"]) if split else np.array_equal(on["bounds"], plain["bounds"])
                for s in range(S):
                    T = len(want[s])
                    assert _bits(on["pcm"][s][:T], want[s]) and not on["pcm"][s][T:].any(), (split, s)
            for gate in (None, trim):  # the stages behind it take the stage's frames: loudness, then conditioning
                on = g.pcm_chain_stretch_host(gate, False, None, st, sr_rates, hz, None, None, S, rates)
                segs = [on["pcm"][s][None, :int(on["frames"][s])] for s in range(S)]
                lalone = _run_stage(g, _loud_spec(), segs, rates, outputs=True)
                with_loud = g.pcm_chain_stretch_host(gate, False, None, st, sr_rates, hz, loud, None, S, rates)
                assert np.array_equal(with_loud["frames"], on["frames"])
                assert _same_records(with_loud["records"], lalone["rec"]) and (with_loud["records"]["status"] == 0).any()
                for s in range(S):
                    T = int(on["frames"][s])
                    assert _bits(with_loud["pcm"][s][:T], lalone["scaled"][s][0]) and not with_loud["pcm"][s][T:].any()
                both = g.pcm_chain_stretch_host(gate, False, None, st, sr_rates, hz, loud, pre, S, rates)
                assert _bits(both["pcm"], _cond_device(g, pre, with_loud["pcm"], with_loud["frames"]))
        # refusals: nothing is written. The need is the largest length on the way: here the stretched one of the slowest segment.
        st = _stretch(64, 16)
        slow = [0.5] * S
        need = max(int(round(int(t) / 0.5)) for t in frames)
        r = np.asarray(slow, np.float64)
        for stride, eff, word in ((need - 1, None, "out_stride_frames"), (need, _effect("harmonic", 64, 16), "not built")):
            out, fr = np.full((S, need), 7.0, np.float32), np.full(S, 7, np.uint64)
            err = C.c_char_p()
            rc = g.lib.vsyn_pcm_chain_stretch_host(g.h, None, 0, None if eff is None else C.byref(eff), C.byref(st), binding._ptr(r), None, None, None, S,
                                                   binding._ptr(binding._rates(rates)), 0, VSYN_PCM_F32, binding._ptr(out), stride, binding._ptr(fr),
                                                   None, None, None, 0, None, None, None, C.byref(err))
            assert rc == binding.VSYN_ERR_INVALID and word in err.value.decode() and (out == 7.0).all(), (word, err.value)
            assert eff is None or (fr == 7).all()
        ok = g.pcm_chain_stretch_host(None, False, None, st, slow, None, None, None, S, rates)
        assert ok["pcm"].shape[1] == need and list(ok["frames"]) == [int(round(int(t) / 0.5)) for t in frames]
        with pytest.raises(VsynError) as ei:
            g.pcm_chain_stretch_host(None, False, None, st, [1.0, 0.0, 1.0][:S], None, None, None, S, rates)
        assert "rate" in str(ei.value)
        f1b, _ = g.pcm_fetch_host(VSYN_PCM_F32, S, b1["plane_stride"])
        assert np.array_equal(f1, f1b)
    finally:
        g.close()


def _ogg(name):
    with open(os.path.join(GOLDEN, name + ".ogg"), "rb") as f:
        return f.read()


def test_files_through_the_chain(synth):
    """get_pcm_batch on test.stereo44khz.ogg and synth_03.ogg: the stretched files are the device entry's output on the same decoded
    PCM, ungated (the stereo planes), behind a trim and behind a split (the gated mono signal), and the loudness normaliser and the
    pre-emphasis behind the stretch are those stages run on its output. pitch_shift returns each file's resampled length."""
    from parseoggvorbis_amd import pcm
    from parseoggvorbis_amd.binding import PcmCond
    blobs = [_ogg("test.stereo44khz"), _ogg("synth_03")]
    n, hop = 256, 64
    rates = [0.9, 1.1]
    kw = dict(mono=True, stretch_n_fft=n, stretch_hop_length=hop)
    planes = pcm.get_pcm_batch(blobs)
    got = pcm.get_pcm_batch(blobs, time_stretch=rates, **kw)
    st = _stretch(n, hop)
    for i, ((x, sr), (y, sr_y)) in enumerate(zip(planes, got)):
        assert sr == sr_y and y.dtype == np.float32 and y.shape == (int(round(x.shape[1] / rates[i])),)
        want = compose(synth, st, [np.ascontiguousarray(x)], [rates[i]])[0]
        assert y.any() and _bits(y, want), i
        assert _bits(y, stage_alone(synth, st, [np.ascontiguousarray(x)], [rates[i]])[0]), i  # the device entry on the same decoded PCM
    one = pcm.get_pcm_batch(blobs, time_stretch=0.9, **kw)  # one rate for every file
    assert _bits(one[0][0], got[0][0]) and one[1][0].shape == (int(round(planes[1][0].shape[1] / 0.9)),)
    assert _bits(pcm.get_pcm_from_raw_bytes(blobs[0], time_stretch=0.9, **kw)[0], got[0][0])
    for gate in (dict(trim_db=30.0, trim_frame_length=256, trim_hop_length=64), dict(split_db=30.0, split_frame_length=256, split_hop_length=64)):
        plain = pcm.get_pcm_batch(blobs, mono=True, **gate)
        on = pcm.get_pcm_batch(blobs, time_stretch=rates, **kw, **gate)
        for i in range(2):
            m = plain[i][0]
            assert on[i][0].shape == (int(round(m.shape[0] / rates[i])),)
            assert _bits(on[i][0], compose(synth, st, [m[None, :]], [rates[i]])[0]), (i, gate)
    # loudness normalisation and pre-emphasis behind the stretch, on the file long enough to be measured
    base = pcm.get_pcm_batch(blobs[:1], time_stretch=rates[:1], **kw)[0]
    lufs = []
    both = pcm.get_pcm_batch(blobs[:1], time_stretch=rates[:1], loudness_normalize=TARGET, loudness=lufs, preemphasis=0.97, **kw)[0]
    alone = _run_stage(synth, _loud_spec(), [base[0][None, :]], [base[1]], outputs=True)
    assert alone["rec"]["status"][0] == 0 and lufs[0] is not None
    scaled = alone["scaled"][0]
    assert _bits(both[0], _cond_device(synth, PcmCond(2, 0, 0.97), np.ascontiguousarray(scaled), [scaled.shape[1]])[0])
    # pitch_shift: rate 2^(-steps / 12), resampled from rint(sr / rate) back to sr, the length kept
    sr = 22050
    rs = pcm.get_pcm_batch(blobs, sr=sr)
    ps = pcm.get_pcm_batch(blobs, sr=sr, pitch_shift=2, **kw)
    rate = 2.0 ** (-2.0 / 12.0)
    sp = _stretch(n, hop, fix=True, to_hz=sr)
    for i in range(2):
        x = rs[i][0]
        assert ps[i][1] == sr and ps[i][0].shape == (x.shape[1],)
        assert _bits(ps[i][0], compose(synth, sp, [np.ascontiguousarray(x)], [rate], _from_hz(sr, [rate]))[0]), i
    # a damaged file fails alone
    bad = bytearray(blobs[0])
    bad[len(bad) // 2] ^= 0x55  # a page CRC
    res = pcm.get_pcm_batch([blobs[0], bytes(bad), blobs[1]], errors="return", files_per_submit=2, time_stretch=[0.9, 1.0, 1.1], **kw)
    assert isinstance(res[1], pcm.PcmError) and "file 1" in str(res[1])
    assert _bits(res[0][0], got[0][0]) and _bits(res[2][0], got[1][0])
