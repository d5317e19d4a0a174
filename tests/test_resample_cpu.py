"""CPU checks of the resampling contract: the float64 model (tests/resample_model.py) against scipy.signal.resample_poly, the
C-ABI's vsyn_resample_num_frames, and the Python argument checks, which run before the library loads."""
import numpy as np
import pytest

import __graft_entry__ as entry
from parseoggvorbis_amd import binding
from tests import resample_model as rm

PAIRS = [(44100, 16000), (48000, 16000), (8000, 16000), (44100, 48000), (22050, 16000), (11025, 44100), (16000, 44100),
         (48000, 44100), (32000, 22050), (11025, 48000), (44056, 16000), (24000, 8000), (16000, 16000), (44100, 44100)]
# 0, 1, shorter than the filter (N = 20 max(up, down) + 1 taps), thousands
LENGTHS = [0, 1, 7, 5000]


@pytest.fixture(scope="module")
def lib():
    entry.build_hip()
    return binding.load()


@pytest.mark.parametrize("r_in,r_out", PAIRS)
def test_model_matches_scipy(r_in, r_out):
    """Measured: largest difference 4.5e-7 over these pairs and lengths (scipy applies float32 taps to float32 input)."""
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(r_in * 7 + r_out)
    up, down = rm.ratio(r_in, r_out)
    for T in LENGTHS:
        x = rng.uniform(-1.0, 1.0, T).astype(np.float32)
        got = rm.resample(x, r_in, r_out)
        assert got.shape == (rm.num_frames(r_in, r_out, T),)
        if T == 0:
            continue  # scipy refuses empty input; the contract gives 0 frames
        want = signal.resample_poly(x, up, down)
        assert want.shape == got.shape, (T, want.shape, got.shape)
        if up == down:
            assert np.array_equal(got.astype(np.float32), x)
        assert np.abs(got - want).max() <= 1e-6, (r_in, r_out, T, np.abs(got - want).max())


def test_model_multichannel_is_per_channel():
    x = np.random.default_rng(3).uniform(-1, 1, (3, 400)).astype(np.float32)
    got = rm.resample(x, 44100, 16000)
    for c in range(3):
        assert np.array_equal(got[c], rm.resample(x[c], 44100, 16000))


def test_taps_sum_to_up():
    for r_in, r_out in PAIRS[:6]:
        up, down = rm.ratio(r_in, r_out)
        assert abs(rm.taps(up, down).sum() - up) < 1e-9 * up


def test_num_frames(lib):
    f = lib.vsyn_resample_num_frames
    for r_in, r_out in PAIRS:
        up, down = rm.ratio(r_in, r_out)
        for T in [0, 1, 2, 7, 441, 5000, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 12345, 3 * 2 ** 40 + 1]:
            assert f(r_in, r_out, T) == -(-T * up // down), (r_in, r_out, T)
    # invalid pairs: a rate of 0, or a reduced M above 65536
    assert f(0, 16000, 100) == 0
    assert f(44100, 0, 100) == 0
    assert f(100003, 16000, 100) == 0  # 100003 is prime: 16000 / 100003
    assert f(16000, 100003, 100) == 0
    assert f(65536, 1, 100) == 1       # M = 65536 is still allowed
    assert f(65537, 1, 100) == 0


def test_python_argument_errors_before_the_library_loads(monkeypatch):
    from parseoggvorbis_amd import pcm, spectral

    def no_load():
        raise AssertionError("library loaded before the arguments were checked")
    monkeypatch.setattr(pcm, "_load", no_load)
    monkeypatch.setattr(spectral, "_load", no_load)
    for sr in (0, -16000, 16000.0, 1.5, "16000", True, 2 ** 32):
        with pytest.raises(pcm.PcmError):
            pcm.get_pcm_batch([b"x"], sr=sr)
        with pytest.raises(spectral.SpectralError):
            spectral.get_spectral_batch([b"x"], sr=sr)
        with pytest.raises(spectral.SpectralError):
            spectral.get_spectral_from_raw_bytes(b"x", sr=sr)
    for dt in ("float64", "int32", "f32", None, np.float64):
        with pytest.raises(pcm.PcmError):
            pcm.get_pcm_batch([b"x"], dtype=dt)
    with pytest.raises(ValueError):
        pcm.get_pcm_batch([b"x"], errors="ignore")
    with pytest.raises(pcm.PcmError):
        pcm.get_pcm_from_raw_bytes(b"x", sr=0)
