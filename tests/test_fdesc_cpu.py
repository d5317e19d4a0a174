"""The frame descriptor stage without a GPU: the float64 model (tests/fdesc_model.py) against a restatement with numpy.fft.rfft and
plain np.cumsum / np.mean, the condition on the test inputs that lets tests/test_gpu_fdesc.py demand every roll-off bin exactly,
the zero-crossing rates of the three signals made for them, and the argument checks of parseoggvorbis_amd.frame_descriptors, which
run before the library is loaded."""
import numpy as np
import pytest

from parseoggvorbis_amd import frame_descriptors as fd
from tests import fdesc_cases as fc
from tests import fdesc_model as fm

IDS = ["%d-%d-%s" % c for c in fc.CONFIGS]


def restate(y, sr, n, hop, win, roll=fc.ROLL, zthr=fc.ZTHR, amin=fc.AMIN):
    """librosa's definitions in its own order of operations, float64: (rows (F, 6), k (F,))."""
    y = np.asarray(y, np.float64)
    F = fm.num_frames(len(y), n, hop)
    if F == 0:
        return np.zeros((0, 6)), np.zeros(0, np.int64)
    P = n // 2
    pick = np.arange(F)[:, None] * hop + np.arange(n)[None, :]
    z0 = np.pad(y, P, mode="constant")
    z0 = np.concatenate([z0, np.zeros(max(0, pick.max() + 1 - len(z0)))])[pick]
    z1 = np.pad(y, P, mode="edge")
    z1 = np.concatenate([z1, np.full(max(0, pick.max() + 1 - len(z1)), y[-1])])[pick]
    rms = np.sqrt(np.mean(z0 ** 2, axis=1))
    z1 = np.where(np.abs(z1) <= zthr, 0.0, z1)
    zcr = np.mean(np.concatenate([np.zeros((F, 1), bool), np.signbit(z1)[:, 1:] != np.signbit(z1)[:, :-1]], axis=1), axis=1)
    S = np.abs(np.fft.rfft(z0 * fm.window(n, n if win is None else win).astype(np.float64)[None, :], axis=1))
    freq = np.arange(n // 2 + 1) * float(sr) / n
    A = S.sum(axis=1)
    live = A >= fm.TINY
    As = np.where(live, A, 1.0)
    cent = np.where(live, (freq * S).sum(axis=1) / As, 0.0)
    bw = np.where(live, np.sqrt((S * (freq[None, :] - cent[:, None]) ** 2).sum(axis=1) / As), 0.0)
    total = np.cumsum(S, axis=1)
    k = np.argmax(total >= (roll * total[:, -1])[:, None], axis=1)
    Pw = np.maximum(amin, S ** 2)
    flat = np.exp(np.mean(np.log(Pw), axis=1)) / np.mean(Pw, axis=1)
    return np.stack([rms, zcr, cent, bw, freq[k], flat], axis=1), k


@pytest.mark.parametrize("n,hop,win", fc.CONFIGS, ids=IDS)
def test_model_agrees_with_the_rfft_restatement(n, hop, win):
    """Every column of every frame of every case within the band (rms, centroid, bandwidth, flatness: band * |model|; zcr and k*
    equal), the restatement being one more float64 evaluation in another order."""
    worst = np.zeros(6)
    for c, m in zip(fc.cases(n, hop, win), fc.models(n, hop, win)):
        rows, k = restate(fc.mono(c), c["sr"], n, hop, win)
        assert rows.shape == m["rows"].shape == (fm.num_frames(c["T"], n, hop), 6)
        if len(k) == 0:
            continue
        assert np.array_equal(rows[:, fm.ZCR], m["rows"][:, fm.ZCR]), (n, hop, c["kind"], c["T"])
        assert np.array_equal(k, m["k"]), (n, hop, c["kind"], c["T"], np.flatnonzero(k != m["k"])[:5])
        for col in (fm.RMS, fm.CENTROID, fm.BANDWIDTH, fm.FLATNESS):
            d = np.abs(rows[:, col] - m["rows"][:, col])
            bound = m["band"][:, col] * np.abs(m["rows"][:, col])
            assert (d <= bound).all(), (n, hop, c["kind"], c["T"], fd.COLUMNS[col], float(d.max()), int(np.argmax(d - bound)))
            nz = bound > 0
            if nz.any():
                worst[col] = max(worst[col], float((d[nz] / bound[nz]).max()))
    print("restatement (n_fft %d, hop %d): worst |d| / bound per column %s" % (n, hop, worst))


@pytest.mark.parametrize("n,hop,win", fc.CONFIGS, ids=IDS)
def test_every_frame_decides_rolloff_outside_the_band(n, hop, win):
    """Every frame of every case has margin > band: a condition on the inputs, no frame left out."""
    least = np.inf
    for c, m in zip(fc.cases(n, hop, win), fc.models(n, hop, win)):
        if len(m["k"]) == 0:
            continue
        b = m["band"][:, fm.ROLLOFF]
        print("margin", n, hop, c["kind"], c["C"], c["T"], c["sr"], float(m["margin"].min()), float(b.max()))
        assert (m["margin"] > b).all(), (n, hop, c["kind"], c["T"], int(np.argmin(m["margin"] - b)), float(m["margin"].min()), float(b.max()))
        least = min(least, float(m["margin"].min()))
        if c["kind"] == "zeros":
            assert (m["k"] == 0).all() and np.isinf(m["margin"]).all() and (m["rows"][:, :5] == 0.0).all()
    assert least < 1.0


@pytest.mark.parametrize("n,hop,win", fc.CONFIGS, ids=IDS)
def test_zero_crossing_rates_of_the_made_signals(n, hop, win):
    """negative_dc: 0 in every frame (edge padding; zero padding would count the step at either end). alternating: (n - 1) / n in
    the frames that lie inside the signal. threshold: the count of a plain loop over the edge-padded frame."""
    for c, m in zip(fc.cases(n, hop, win), fc.models(n, hop, win)):
        if c["T"] != fc.T_MID:
            continue
        zcr, y = m["rows"][:, fm.ZCR], fc.mono(c).astype(np.float64)
        starts = np.arange(len(zcr)) * hop - n // 2
        inside = (starts >= 0) & (starts + n <= c["T"])
        if c["kind"] == "negative_dc":
            assert (zcr == 0.0).all()
            zero_padded = fm.frames_of(fc.mono(c), n, hop)
            assert ((zero_padded[0] < 0) != (zero_padded[0, 0] < 0)).any()  # (what zero padding would have counted)
        elif c["kind"] == "alternating":
            assert (inside.any() or c["T"] < 2 * n) and (zcr[inside] == (n - 1) / float(n)).all()
            assert (zcr[~inside] <= (n - 1) / float(n)).all()
        elif c["kind"] == "threshold":
            for f in sorted({0, len(zcr) // 2, len(zcr) - 1}):
                count, prev = 0, None
                for j in range(n):
                    v = y[min(max(int(starts[f]) + j, 0), c["T"] - 1)]
                    s = bool(v < 0.0 and abs(v) > fc.ZTHR)
                    count += int(prev is not None and s != prev)
                    prev = s
                assert zcr[f] == count / float(n) and (count > 0 or f != len(zcr) // 2), (n, hop, f, count)


def test_frame_counts_and_refusal():
    for n, hop, win in fc.CONFIGS:
        for T in fc.lengths(n, hop):
            assert fm.num_frames(T, n, hop) == (0 if T == 0 else 1 + (T + 2 * (n // 2) - n) // hop)
    y = np.ones(300, np.float32)
    y[7] = np.inf
    m = fm.describe(y, 8000, 64, 200)
    assert m["refused"] and m["rows"].shape == (2, 6) and np.isnan(m["rows"]).all()


def test_fixture_frames_that_decide_rolloff_inside_the_band_are_few():
    """The reference decoder's PCM of the Ogg fixtures (tests/golden/<name>.npz, what tests/test_oracle_golden.py decodes) through
    the model at the end-to-end test's n_fft = 512, hop = 160: the frames whose roll-off margin is not above the band, which
    tests/test_gpu_fdesc.py lets take a neighbouring bin, stay under its cap of 1 %."""
    import os
    import struct
    from tests import trim_model as tm
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    names = ["test.stereo44khz", "test.mono44khz"] + ["synth_%02d" % i for i in range(16)] + ["winflags_bcd"]  # tests/test_gpu_spectral.py: FILES
    frames = marginal = 0
    for name in names:
        x = np.load(os.path.join(golden, name + ".npz"))["pcm"]
        data = open(os.path.join(golden, name + ".ogg"), "rb").read()
        sr = struct.unpack_from("<I", data, 27 + data[26] + 12)[0]
        m = fm.describe(tm.downmix(x) if x.shape[1] else np.zeros(0, np.float32), sr, 512, 160)
        frames += len(m["k"])
        marginal += int((~(m["margin"] > m["band"][:, fm.ROLLOFF])).sum())
    print("fixtures: %d of %d frames decide roll-off inside the band" % (marginal, frames))
    assert frames > 0 and marginal <= 0.01 * frames


BAD = [dict(n_fft=15), dict(n_fft=8193), dict(n_fft=2048.0), dict(n_fft=True), dict(hop_length=0), dict(hop_length=2 ** 32),
       dict(hop_length=1.5), dict(hop_length=None), dict(win_length=0), dict(win_length=2049), dict(win_length=1.5), dict(center=1),
       dict(roll_percent=0.0), dict(roll_percent=1.0), dict(roll_percent=float("nan")), dict(roll_percent="0.85"),
       dict(zcr_threshold=-1e-3), dict(zcr_threshold=float("inf")), dict(zcr_threshold=None), dict(amin=0.0), dict(amin=-1.0),
       dict(amin=float("nan")), dict(amin=True), dict(sr=0), dict(sr=16000.0), dict(errors="ignore"), dict(threads=-1), dict(feeders=1.5),
       dict(device="0"), dict(files_per_submit=0)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join("%s=%r" % kv for kv in kw.items()))
def test_bad_arguments_are_refused_before_the_library_loads(kw, monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(fd, "_load", no_load)
    with pytest.raises(fd.FrameDescriptorError):
        fd.get_frame_descriptors_batch([b"x"], **kw)
    spec_kw = {k: v for k, v in kw.items() if k in ("n_fft", "hop_length", "win_length", "center", "roll_percent", "zcr_threshold", "amin")}
    if spec_kw:
        with pytest.raises(fd.FrameDescriptorError):
            fd.fdesc_spec(**spec_kw)


def test_spec_defaults():
    s = fd.fdesc_spec()
    assert (s.n_fft, s.hop_length, s.win_length, s.options, s.roll_percent, s.zcr_threshold, s.amin) == (2048, 512, 2048, 1, 0.85, 1e-10, 1e-10)
    s = fd.fdesc_spec(1024, 256, 700, center=False, roll_percent=0.5)
    assert (s.n_fft, s.hop_length, s.win_length, s.options, s.roll_percent) == (1024, 256, 700, 0, 0.5)
    assert fd.COLUMNS == ("rms", "zcr", "centroid", "bandwidth", "rolloff", "flatness") and issubclass(fd.FrameDescriptorError, RuntimeError)
