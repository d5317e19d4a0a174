"""What the loudness stage (include/vorbis_synth_hip.h, "loudness") needs without a GPU: the float64 model of tests/loudness_model.py
pinned to the standard (BS.1770-4's coefficient table, its 997 Hz calibration, EBU Tech 3341 cases 1 to 5), the integer hops at rates
that are no multiple of 10, the host library's coefficients and matrix powers against the model's, the NumPy restatement of the
device's blocked order and a sequential evaluation in np.longdouble inside the bound of DESIGN.md 6m, the struct layouts, and the
Python layer's argument checks before the library loads."""
import ctypes as C
import math

import numpy as np
import pytest

from parseoggvorbis_amd import loudness  # (imports without the library: the argument checks below run before it loads)
from tests import loudness_model as lm

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz), as printed: 14 decimals
BS1770_48K = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
              1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]


def test_coefficients_at_48k_are_the_standards_table():
    d = np.abs(np.array(lm.coefficients(48000)) - np.array(BS1770_48K)).max()
    print("48 kHz coefficients against BS.1770-4's table: %.3g" % d)
    assert d < 1e-14  # half a unit of the table's last digit is 5e-15


def _sine(f, fs, seconds, dbfs, channels=1):
    t = np.arange(int(round(seconds * fs))) / fs
    x = (10.0 ** (dbfs / 20.0)) * np.sin(2.0 * np.pi * f * t)
    return np.repeat(x[None, :], channels, axis=0).astype(np.float32)


def test_997_hz_calibration():
    m = lm.measure(_sine(997.0, 48000, 10.0, 0.0), 48000)
    print("997 Hz at 0 dBFS, mono: %.4f LUFS" % m["lufs"])
    assert abs(m["lufs"] - (-3.01)) < 0.01


EBU_3341 = {
    1: ([(20.0, -23.0)], -23.0),
    2: ([(20.0, -33.0)], -33.0),
    3: ([(10.0, -36.0), (60.0, -23.0), (10.0, -36.0)], -23.0),
    4: ([(10.0, -72.0), (10.0, -36.0), (60.0, -23.0), (10.0, -36.0), (10.0, -72.0)], -23.0),
    5: ([(20.0, -26.0), (20.1, -20.0), (20.0, -26.0)], -23.0),
}


@pytest.mark.parametrize("case", sorted(EBU_3341))
def test_ebu_tech_3341(case):
    """1 kHz stereo sine, the same signal in both channels, 48 kHz; each within the document's own +-0.1 LU."""
    parts, want = EBU_3341[case]
    fs = 48000
    n = [int(round(sec * fs)) for sec, _ in parts]
    t = np.arange(sum(n)) / fs
    amp = np.concatenate([np.full(k, 10.0 ** (db / 20.0)) for k, (_, db) in zip(n, parts)])
    x = (amp * np.sin(2.0 * np.pi * 1000.0 * t)).astype(np.float32)
    m = lm.measure(np.stack([x, x]), fs)
    print("EBU Tech 3341 case %d: %.3f LUFS (target %.1f), margins %.3g / %.3g" % (case, m["lufs"], want, *m["margins"]))
    assert m["status"] == lm.OK and abs(m["lufs"] - want) <= 0.1
    assert min(m["margins"]) > 0.1  # no decision near a rounding
    assert lm.margins_exceed(m, fs, float(np.abs(x).max()))


@pytest.mark.parametrize("fs", [11025, 22050, 44100, 8000])
def test_hops_tile_the_signal_at_any_rate(fs):
    for T in (0, fs // 10, 4 * fs // 10 + 1, 3 * fs + 17, 10 * fs - 1):
        e = lm.hop_edges(fs, T)
        Nh = lm.num_hops(fs, T)
        assert len(e) == Nh + 1 and e[0] == 0 and e[-1] == (Nh * fs) // 10 <= T
        assert T - e[-1] < fs / 10.0 + 1  # the tail is shorter than a hop
        assert (np.diff(e) > 0).all()  # no gap, no overlap: consecutive edges
        if Nh >= 4:
            n = e[4:] - e[:-4]
            assert n.max() - n.min() <= 1, (fs, T)
            assert lm.num_blocks(fs, T) == Nh - 3
        if fs % 10 == 0:
            assert (np.diff(e) == fs // 10).all()


def test_four_hops_is_the_shortest_measured_segment():
    assert loudness.MIN_RATE == lm.MIN_RATE and loudness.STATUS_SILENT == lm.SILENT  # the Python layer's constants are the model's
    for fs in lm.RATES:
        h4 = (4 * fs + 9) // 10
        assert lm.num_hops(fs, h4) == 4 and lm.num_hops(fs, h4 - 1) == 3
        x = lm.signal("noise", 1, h4, 1)
        assert lm.measure(x, fs)["status"] == lm.OK and lm.measure(x[:, :-1], fs)["status"] == lm.TOO_SHORT
    assert lm.measure(lm.signal("noise", 1, 4000, 1), 3999)["status"] == lm.RATE_REFUSED


def test_statuses_and_gates_of_the_model():
    fs = 8000
    T = 3 * fs
    assert lm.measure(lm.signal("zeros", 2, T, 0), fs)["status"] == lm.SILENT
    assert lm.measure(lm.signal("zeros", 2, T, 0), fs)["lufs"] == -math.inf
    g = lm.measure(lm.signal("gated", 2, T, 5), fs)
    assert g["status"] == lm.OK and g["blocks"] > g["blocks_abs"] > g["blocks_rel"] > 0  # both gates cut
    x = lm.signal("noise", 1, T, 2)
    x[0, T - 3] = np.nan  # in the tail behind the last whole hop? (T is whole hops here: in the last hop)
    assert lm.measure(x, fs)["status"] == lm.NOT_FINITE
    x = lm.signal("noise", 1, T + 5, 2)
    x[0, T + 2] = np.inf  # the tail behind the last whole hop
    assert lm.measure(x, fs)["status"] == lm.NOT_FINITE
    # the gain reproduces from zbar alone
    m = lm.measure(lm.signal("noise", 2, T, 3), fs, target=-23.0)
    assert m["gain"] == np.float32(np.sqrt(10.0 ** ((-23.0 + 0.691) / 10.0) / m["zbar"]))
    # mono is the float32 downmix of "PCM conditioning"
    x = lm.signal("noise", 2, T, 4)
    assert np.array_equal(lm.downmix(x)[0], ((x[0] + x[1]) * np.float32(0.5)))


# ---- the host library's tables (no GPU needed: the library loads without one) ----
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    from parseoggvorbis_amd import binding
    entry.build_hip()
    return binding.load()


@pytest.mark.parametrize("fs", [4000, 8000, 11025, 16000, 22050, 44100, 48000, 96000, 192000])
def test_host_coefficients_and_powers(lib, fs):
    """The coefficients bit for bit; every element of the host's A^(32 2^k) within one rounding of the exact power (the model's
    powers() are the exact integer powers correctly rounded; on the build machine the host's are those, bit for bit)."""
    k = np.zeros(10)
    assert lib.vsyn_loudness_coefficients(fs, k.ctypes.data) == 0
    assert np.array_equal(k, np.array(lm.coefficients(fs)))
    M = np.zeros(16 * (lm.LEVELS + 1))
    assert lib.vsyn_loudness_powers(fs, M.ctypes.data) == 0
    W = np.array(lm.powers(lm.coefficients(fs))).reshape(-1)
    assert (np.abs(M - W) <= lm.U * np.abs(W) + 2.0 ** -1074).all()
    assert lib.vsyn_loudness_coefficients(3999, k.ctypes.data) != 0 and lib.vsyn_loudness_powers(fs, None) != 0
    assert lib.vsyn_loudness_num_blocks(fs, (4 * fs + 9) // 10) == 1 and lib.vsyn_loudness_num_blocks(fs, (4 * fs + 9) // 10 - 1) == 0
    assert lib.vsyn_loudness_num_blocks(3999, 10 ** 6) == 0
    assert lib.vsyn_loudness_num_blocks(fs, 7 * fs + 3) == lm.num_blocks(fs, 7 * fs + 3)


def test_struct_layouts():
    from parseoggvorbis_amd import binding
    assert C.sizeof(binding.LoudnessSpec) == 16 and binding.LoudnessSpec.target.offset == 8
    d = binding.LOUDNESS_RECORD_DTYPE
    assert d.itemsize == 40 and d.fields["blocks"][1] == 16 and d.fields["gain"][1] == 28 and d.fields["status"][1] == 32


# ---- the bound ----
@pytest.mark.parametrize("fs", [8000, 11025, 48000, 192000])
def test_blocked_order_and_longdouble_inside_the_bound(fs):
    """Measured here, worst |dy| over noise and noise on a DC offset of 0.5, three tiles and 77 samples, as a fraction of the gate
    (seq + dev) X: 8 kHz 2.9e-3, 11 025 Hz 3.1e-3, 48 kHz 1.1e-3, 192 kHz 5.7e-4. The bound is a worst case over the signs of
    every rounding; the error itself grows like a random walk. Against np.longdouble (20 000 samples): the model at most 3.0e-3 of
    its half, the blocked order at most 2.9e-3 of its own."""
    b = lm.bounds(fs)
    worst = 0.0
    for kind in ("noise", "dc"):
        x = lm.signal(kind, 1, 3 * lm.TILE + 77, 3)[0]
        X = float(np.abs(x).max())
        d = float(np.abs(lm.blocked(x, fs) - lm.kweight(x, fs)).max())
        worst = max(worst, d / lm.sample_bound(fs, X))
        print("%6d Hz %-5s max |dy| %.3g = %.3g of the gate, %.3g of 2^-53 norm1(h) X" % (fs, kind, d, d / lm.sample_bound(fs, X),
                                                                                         d / (lm.U * b["norm1"] * X)))
    assert 0.0 < worst <= 1.0
    if np.finfo(np.longdouble).eps < 2.0 ** -60:  # something more exact than the model exists on this machine
        x = lm.signal("dc", 1, 20000, 9)[0]
        X = float(np.abs(x).max())
        yl = lm.sequential_longdouble(x, fs)
        r_seq = float(np.abs(lm.kweight(x, fs) - yl).max()) / (b["seq"] * X)
        r_dev = float(np.abs(lm.blocked(x, fs) - yl).max()) / (b["dev"] * X)
        print("%6d Hz against longdouble: model %.3g of seq, blocked %.3g of dev" % (fs, r_seq, r_dev))
        assert 0.0 < r_seq <= 1.0 and 0.0 < r_dev <= 1.0


def test_the_all_pole_norm_drives_the_bound():
    """The double pole of the high pass near z = 1: the l1 norm of its all-pole part grows like 1 / (1 - rho)^2 (4.0e4 at 48 kHz,
    6.4e5 at 192 kHz), and so do both halves of the bound; norm1(h) of the whole filter stays near 3.3."""
    a, b = lm.bounds(48000), lm.bounds(192000)
    assert 3.9e4 < a["allpole"] < 4.2e4 and 6.2e5 < b["allpole"] < 6.6e5
    assert 3.0 < a["norm1"] < 3.6 and 3.0 < b["norm1"] < 3.6
    assert b["seq"] > 10 * a["seq"] and b["dev"] > 10 * a["dev"]


def test_blocked_order_is_independent_of_what_follows():
    """The decomposition counts from the segment's first sample: a prefix gives the bits of the whole."""
    x = lm.signal("dc", 1, 2 * lm.TILE + 5, 11)[0]
    y = lm.blocked(x, 48000)
    for n in (lm.SUB + 1, lm.TILE, lm.TILE + 1):
        assert np.array_equal(lm.blocked(x[:n], 48000), y[:n])


# ---- the Python layer: every refusal before the library loads ----
BAD_LOUDNESS = [dict(channels="left"), dict(channels=None), dict(channels=1), dict(blocks=1), dict(blocks="yes"), dict(sr=0), dict(sr=3999),
                dict(sr=16000.0), dict(sr=True), dict(errors="ignore")]
BAD_NORMALIZE = [dict(loudness_normalize=0.5), dict(loudness_normalize=-70.5), dict(loudness_normalize=float("nan")),
                 dict(loudness_normalize=float("-inf")), dict(loudness_normalize="-23"), dict(loudness_normalize=True),
                 dict(loudness_normalize=-23.0, peak_normalize=True), dict(loudness_normalize=-23.0, loudness=()),
                 dict(loudness={}), dict(loudness_normalize=[-23.0])]


def _no_load():
    raise AssertionError("library loaded before the arguments were checked")


def _ids(kw):
    return "-".join("%s=%r" % it for it in kw.items())


@pytest.mark.parametrize("kw", BAD_LOUDNESS, ids=_ids)
def test_bad_loudness_keywords_raise_before_the_library_loads(kw, monkeypatch):
    from parseoggvorbis_amd import loudness
    monkeypatch.setattr(loudness, "_load", _no_load)
    with pytest.raises((loudness.LoudnessError, ValueError)):
        loudness.get_loudness_batch([b"OggS"], **kw)
    with pytest.raises((loudness.LoudnessError, ValueError)):
        loudness.get_loudness_from_raw_bytes(b"OggS", **kw)


@pytest.mark.parametrize("kw", BAD_NORMALIZE, ids=_ids)
def test_bad_normaliser_keywords_raise_before_the_library_loads(kw, monkeypatch):
    from parseoggvorbis_amd import pcm, spectral
    monkeypatch.setattr(pcm, "_load", _no_load)
    monkeypatch.setattr(spectral, "_load", _no_load)
    with pytest.raises(pcm.PcmError):
        pcm.get_pcm_batch([b"OggS"], mono=True, **kw)
    with pytest.raises(spectral.SpectralError):
        spectral.get_spectral_batch([b"OggS"], n_fft=64, hop_length=16, n_mels=8, **kw)


def test_the_normaliser_needs_mono_and_good_keywords_reach_the_library(monkeypatch):
    from parseoggvorbis_amd import loudness, pcm, spectral

    class Reached(Exception):
        pass

    def reached():
        raise Reached()
    for mod in (loudness, pcm, spectral):
        monkeypatch.setattr(mod, "_load", reached)
    with pytest.raises(pcm.PcmError) as ei:
        pcm.get_pcm_batch([b"OggS"], loudness_normalize=-23.0)
    assert "mono=True" in str(ei.value)
    got = []
    for t in (-70, 0, -23.0, np.float32(-16.0)):
        with pytest.raises(Reached):
            pcm.get_pcm_batch([b"OggS"], mono=True, loudness_normalize=t, loudness=got, sr=16000, trim_db=40.0, preemphasis=0.97)
        with pytest.raises(Reached):
            spectral.get_spectral_batch([b"OggS"], loudness_normalize=t, loudness=got, split_db=40.0, delta=1, normalize="mean")
    with pytest.raises(Reached):
        spectral.get_spectral_batch([b"OggS"], kind="mel_power", pcen=True, loudness_normalize=-23.0)
    for kw in (dict(), dict(sr=4000), dict(channels="mono", blocks=True), dict(channels="sum", sr=16000)):
        with pytest.raises(Reached):
            loudness.get_loudness_batch([b"OggS"], **kw)
    s = loudness.loudness_spec("mono", -23)
    assert (s.options, s.channel_mode, s.target) == (1, 1, -23.0)
    s = loudness.loudness_spec()
    assert (s.options, s.channel_mode, s.target) == (0, 0, 0.0)
    assert loudness.lufs_of(0.0) == -math.inf and abs(float(loudness.lufs_of(1.0)) + 0.691) < 1e-15
