"""The beat tracker on the device (include/vorbis_synth_hip.h, "rhythm", D) against the float64 model of tests/beat_model.py, through
vsyn_beat_track_device on the shared cases of tests/beat_cases.py, and the host chain from Ogg bytes against the device form.

Gates (tests/beat_model.py derives them): every local score within LSB and every cumulative score within CB of the model's, per value;
the back links, the beats and the counts equal to the model's (tests/test_beat_cpu.py asserts that every case decides every comparison
beyond the band two correct evaluations can differ in). The same envelope gives the same bits anywhere in a batch, next to segments of
other periods, with and without the three optional outputs. The host chain adds no arithmetic: its beats are the device form's on the
envelope get_onset_strength_batch returns, with the period of the tempo get_tempo_batch returns, bit for bit. Each test prints its
worst |d| / bound under pytest -s."""
import numpy as np
import pytest

from tests import beat_cases as bc
from tests import rhythm_model as rm

pytestmark = pytest.mark.gpu

FILL = 0xDEADBEEF - (1 << 32)
TINY = 2.0 ** -1022


@pytest.fixture(scope="module")
def synth():
    import torch
    assert torch.cuda.is_available()
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    yield g
    g.close()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _spec(tightness=100.0, trim=True, start_bpm=120.0, bpm=0.0, hop=512):
    from parseoggvorbis_amd import binding
    return binding.BeatSpec(tightness, start_bpm, bpm, hop, 1 if trim else 0)


def _run(g, spec, envs, periods, optional=True, expect_error=False):
    """vsyn_beat_track_device over the envelopes back to back: one dict a segment (beats int64 or None where the count was not
    written, count, refused, ls, cum, back as the device left them). Everything is filled with sentinels first: what lies behind an
    output, behind a segment's count and in a segment that has no score must keep them, and the envelopes are read only."""
    import torch
    x = np.concatenate(envs) if envs else np.zeros(0, np.float32)
    n, S = len(x), len(envs)
    d_env = torch.from_numpy(np.ascontiguousarray(x)).cuda() if n else torch.zeros(1, device="cuda")
    d_beats = torch.full((n + 3,), FILL, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((S + 1,), FILL, dtype=torch.int32, device="cuda")
    d_ref = torch.full((S + 1,), FILL, dtype=torch.int32, device="cuda")
    d_ls = torch.full((n + 3,), float("nan"), dtype=torch.float64, device="cuda")
    d_cum = torch.full((n + 3,), float("nan"), dtype=torch.float64, device="cuda")
    d_back = torch.full((n + 3,), FILL, dtype=torch.int32, device="cuda")
    opt = (d_ls.data_ptr(), d_cum.data_ptr(), d_back.data_ptr()) if optional else (None, None, None)
    failed = None
    try:
        g.beat_track_device(spec, [len(e) for e in envs], periods, d_env.data_ptr(), d_beats.data_ptr(), d_cnt.data_ptr(), d_ref.data_ptr(), *opt,
                            stream=_stream())
    except Exception as e:  # noqa: BLE001 (handed back below)
        failed = e
    finally:
        torch.cuda.synchronize()
    beats, cnt, ref = d_beats.cpu().numpy(), d_cnt.cpu().numpy(), d_ref.cpu().numpy()
    ls, cum, back = d_ls.cpu().numpy(), d_cum.cpu().numpy(), d_back.cpu().numpy()
    assert cnt[S] == FILL and ref[S] == FILL and np.all(beats[n:] == FILL) and np.isnan(ls[n:]).all() and np.isnan(cum[n:]).all() and np.all(back[n:] == FILL)
    if n:
        assert np.array_equal(d_env.cpu().numpy(), x, equal_nan=True)
    if failed is not None:
        assert expect_error, failed
        assert np.all(beats == FILL) and np.all(cnt == FILL) and np.all(ref == FILL) and np.isnan(ls).all() and np.isnan(cum).all() and np.all(back == FILL)
        raise failed
    assert not expect_error
    offs = np.concatenate([[0], np.cumsum([len(e) for e in envs])]).astype(np.int64)
    out = []
    for i in range(S):
        a, b = offs[i], offs[i + 1]
        seg = dict(count=int(cnt[i]), refused=int(ref[i]), ls=ls[a:b], cum=cum[a:b], back=back[a:b], beats=None)
        if cnt[i] != FILL:
            assert 0 <= cnt[i] <= len(envs[i])
            assert np.all(beats[a + cnt[i]:b] == FILL)
            seg["beats"] = beats[a:a + cnt[i]].astype(np.int64)
        else:
            assert np.all(beats[a:b] == FILL)
        out.append(seg)
    return out


def _gate(seg, r):
    """One segment against the model's result r; returns the worst |d| / bound of ls and of cum."""
    assert seg["refused"] == r["refused"] and seg["count"] == len(r["beats"])
    assert np.array_equal(seg["beats"], r["beats"])
    if not r["scored"]:  # nothing of a segment without a score is written
        assert np.isnan(seg["ls"]).all() and np.isnan(seg["cum"]).all() and np.all(seg["back"] == FILL)
        return 0.0, 0.0
    dl, dc = np.abs(seg["ls"] - r["ls"]), np.abs(seg["cum"] - r["cum"])
    assert np.all(dl <= r["LSB"] + TINY), float((dl / (r["LSB"] + TINY)).max())
    assert np.all(dc <= r["CB"] + TINY), float((dc / (r["CB"] + TINY)).max())
    assert np.array_equal(seg["back"], r["back"])
    return float((dl / (r["LSB"] + TINY)).max()), float((dc / (r["CB"] + TINY)).max())


@pytest.mark.parametrize("name", bc.names())
def test_case_against_the_model(synth, name):
    _, x, P, tight, trim = bc.case(name)
    seg = _run(synth, _spec(tight, trim), [x], [P])[0]
    wl, wc = _gate(seg, bc.model(name))
    print("beats %s: %d beats, worst |d| / bound ls %.3f cum %.3f" % (name, seg["count"], wl, wc))


def _same(a, b):
    for k in ("count", "refused"):
        assert a[k] == b[k], k
    assert (a["beats"] is None) == (b["beats"] is None) and (a["beats"] is None or np.array_equal(a["beats"], b["beats"]))
    for k in ("ls", "cum", "back"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_same_envelope_same_bits_in_a_mixed_batch(synth):
    """Several cases in one call with a refused (NaN) segment and a skipped (P = 0) one: each segment is gated against the model, is
    what it is alone bit for bit, and is that again at another place, next to other periods, and without the optional outputs. The NaN
    segment is refused alone (word 1, count 0); the skipped one has nothing written, count and word included."""
    picks = bc.mixed_batch()
    segs = [bc.batch_segment(n) for n in picks]
    envs, periods = [s[0] for s in segs], [s[1] for s in segs]
    spec = _spec()
    got = _run(synth, spec, envs, periods)
    alone = {}
    for n, e, P, s in zip(picks, envs, periods, got):
        if n == "nan":
            assert (s["count"], s["refused"]) == (0, 1) and np.isnan(s["ls"]).all() and np.all(s["back"] == FILL)
        elif n == "skipped":
            assert (s["count"], s["refused"]) == (FILL, FILL) and s["beats"] is None and np.isnan(s["ls"]).all() and np.isnan(s["cum"]).all()
            assert np.all(s["back"] == FILL)
        else:
            _gate(s, bc.model(n))
            if n not in alone:
                alone[n] = _run(synth, spec, [e], [P])[0]
            _same(s, alone[n])
    assert len(got[0]["beats"]) == 30 and picks[0] == picks[10] == "clicks20"
    order = list(range(len(picks)))[::-1]
    back = _run(synth, spec, [envs[i] for i in order], [periods[i] for i in order])
    for k, i in enumerate(order):
        _same(back[k], got[i])
    bare = _run(synth, spec, envs, periods, optional=False)
    for s, b in zip(got, bare):
        assert s["count"] == b["count"] and s["refused"] == b["refused"]
        assert (s["beats"] is None) == (b["beats"] is None) and (s["beats"] is None or np.array_equal(s["beats"], b["beats"]))
        assert np.isnan(b["ls"]).all() and np.isnan(b["cum"]).all() and np.all(b["back"] == FILL)
    # a period above 2048 refuses its segment with word 3; a call of skipped segments alone launches nothing
    w = _run(synth, spec, [envs[0], envs[1]], [2049, periods[1]])
    assert (w[0]["count"], w[0]["refused"]) == (0, 3) and np.isnan(w[0]["ls"]).all()
    _same(w[1], got[1])
    z = _run(synth, spec, [envs[0], envs[1]], [0, 0])
    assert z[0]["count"] == z[1]["count"] == FILL


def test_refusals_leave_the_outputs_alone(synth):
    from parseoggvorbis_amd import binding
    x = rm.click_train()
    for kw in (dict(tightness=0.0), dict(tightness=-1.0), dict(tightness=np.nan), dict(tightness=np.inf), dict(start_bpm=0.0),
               dict(start_bpm=np.nan), dict(bpm=-1.0), dict(bpm=np.inf), dict(hop=0)):
        with pytest.raises(binding.VsynError) as ei:
            _run(synth, _spec(**kw), [x], [20], expect_error=True)
        assert ei.value.code == binding.VSYN_ERR_INVALID, kw
    bad = _spec()
    bad.options = 2
    with pytest.raises(binding.VsynError):
        _run(synth, bad, [x], [20], expect_error=True)


# ---- the host chain, from Ogg bytes --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from parseoggvorbis_amd import rhythm
    return rhythm


@pytest.fixture(scope="module")
def blobs():
    """The two real fixtures, and the mono one re-headed to 16 kHz so that the rates differ within a call."""
    from tests.test_gpu_spectral import _ogg, _rehead
    real = [_ogg("test.stereo44khz"), _ogg("test.mono44khz")]
    return real + [_rehead(real[1], 16000)]


SMALL = dict(n_fft=400, hop_length=160, n_mels=40)
E2E = [dict(), dict(sr=16000), dict(trim_db=30.0), dict(SMALL, kind="mel_power", hpss="percussive", sr=16000, trim_db=30.0)]
OKW = dict(lag=2, max_size=3)


def _device_beats(g, env, bpm, rate, hop, **kw):
    """The device form on one envelope with the period of one tempo: the beats, int64."""
    from parseoggvorbis_amd import binding
    spec = _spec(hop=hop, **kw)
    P = binding.beat_period(spec, bpm, rate)
    assert 1 <= P <= 2048
    seg = _run(g, spec, [env], [P])[0]
    assert seg["refused"] == 0
    return seg["beats"]


@pytest.mark.parametrize("kw", E2E, ids=lambda k: "-".join("%s=%s" % (a, k[a]) for a in ("kind", "sr", "trim_db", "hpss") if a in k) or "defaults")
def test_end_to_end_from_ogg_bytes(synth, mods, blobs, kw):
    """bpm is get_tempo_batch's, bit for bit; the beats are the device form's on the envelope get_onset_strength_batch returns with
    that tempo's period, bit for bit; the same with a caller's bpm, one number and a list."""
    from tests.test_gpu_spectral import _rate
    rhythm = mods
    hop = kw.get("hop_length", 512)
    rates = [kw.get("sr") or _rate(b) for b in blobs]
    tempo = rhythm.get_tempo_batch(blobs, **OKW, **kw)
    env = rhythm.get_onset_strength_batch(blobs, **OKW, **kw)
    envs = []
    beats = rhythm.get_beats_batch(blobs, envelope=envs, **OKW, **kw)
    for i, (bpm, b, sr) in enumerate(beats):
        assert (bpm, sr) == tempo[i] and sr == rates[i] and b.dtype == np.int64
        assert np.array_equal(envs[i], env[i])
        assert np.array_equal(b, _device_beats(synth, env[i], bpm, sr, hop)) and len(b) >= 1
        assert np.all(np.diff(b) > 0) and b[-1] < len(env[i])
    loose = rhythm.get_beats_batch(blobs, tightness=1.0, trim=False, start_bpm=90.0, **OKW, **kw)
    slow = rhythm.get_tempo_batch(blobs, start_bpm=90.0, **OKW, **kw)
    for i, (bpm, b, sr) in enumerate(loose):
        assert (bpm, sr) == slow[i]
        assert np.array_equal(b, _device_beats(synth, env[i], bpm, sr, hop, tightness=1.0, trim=False))
    fixed = rhythm.get_beats_batch(blobs, bpm=100.0, **OKW, **kw)
    listed = rhythm.get_beats_batch(blobs, bpm=[100.0, 140.0, 100.0], **OKW, **kw)
    for i, want_bpm in enumerate((100.0, 140.0, 100.0)):
        assert fixed[i][0] == 100.0 and listed[i][0] == want_bpm and fixed[i][2] == listed[i][2] == rates[i]
        assert np.array_equal(fixed[i][1], _device_beats(synth, env[i], 100.0, rates[i], hop))
        assert np.array_equal(listed[i][1], _device_beats(synth, env[i], want_bpm, rates[i], hop))
    one = rhythm.get_beats_from_raw_bytes(blobs[1], **OKW, **kw)
    assert one[0] == beats[1][0] and np.array_equal(one[1], beats[1][1]) and one[2] == beats[1][2]
    print("beats end to end %r: %r" % (kw, [(round(t[0], 3), len(t[1]), t[2]) for t in beats]))


def test_a_damaged_file_fails_alone_and_the_other_entries_are_unchanged(mods, blobs):
    rhythm = mods
    names = [0, 1, 2] * 2
    data = [blobs[i] for i in names]
    bad = bytearray(data[4])
    bad[len(bad) // 2] ^= 0x55  # a page CRC
    data[4] = bytes(bad)
    onsets_before = rhythm.get_onsets_batch(blobs)
    tempo_before = rhythm.get_tempo_batch(blobs)
    single = [rhythm.get_beats_from_raw_bytes(b) for b in blobs]
    res = rhythm.get_beats_batch(data, errors="return", files_per_submit=4)
    listed = rhythm.get_beats_batch(data, errors="return", files_per_submit=4, bpm=[100.0, 100.0, 120.0, 100.0, 120.0, 100.0])
    for i, n in enumerate(names):
        if i == 4:
            assert isinstance(res[i], rhythm.RhythmError) and "file 4" in str(res[i])
            assert isinstance(listed[i], rhythm.RhythmError) and "file 4" in str(listed[i])
            continue
        assert res[i][0] == single[n][0] and np.array_equal(res[i][1], single[n][1]) and res[i][2] == single[n][2]
        assert isinstance(listed[i], tuple) and listed[i][0] == (120.0 if i == 2 else 100.0)
    with pytest.raises(rhythm.RhythmError):
        rhythm.get_beats_batch(data)
    # a tempo window length outside [2, 2048] fails that file alone (8 s at 44100 / 160 are 2205 frames, at 16000 / 160 800), and so
    # does a beat period outside [1, 2048] frames (1 bpm at 44100 / 512 are 5168 frames, at 16000 / 512 1875)
    t = rhythm.get_beats_batch(blobs, errors="return", n_fft=400, hop_length=160, n_mels=40)
    assert isinstance(t[0], rhythm.RhythmError) and isinstance(t[1], rhythm.RhythmError) and "[2, 2048]" in str(t[0]) and isinstance(t[2], tuple)
    t = rhythm.get_beats_batch(blobs, errors="return", bpm=1.0)
    assert isinstance(t[0], rhythm.RhythmError) and isinstance(t[1], rhythm.RhythmError) and "beat period" in str(t[0]) and isinstance(t[2], tuple)
    assert t[2][0] == 1.0
    # one frame a file (a hop longer than the file): not refused, no beats, and the chain reports bpm 0.0
    t = rhythm.get_beats_batch(blobs[:2], hop_length=1 << 20, bpm=1.0)
    assert [(bpm, len(b), b.dtype, sr) for bpm, b, sr in t] == [(0.0, 0, np.int64, 44100)] * 2
    # the entries this one stands beside return what they returned before it ran
    onsets_after = rhythm.get_onsets_batch(blobs)
    tempo_after = rhythm.get_tempo_batch(blobs)
    assert tempo_after == tempo_before and all(np.array_equal(a, b) for a, b in zip(onsets_after, onsets_before))
