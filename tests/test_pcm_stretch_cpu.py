"""The Python rules of get_pcm_batch's time_stretch / pitch_shift arguments (parseoggvorbis_amd/pcm.py, stretch_args): no GPU and no
library."""
import numpy as np
import pytest


class _Reached(Exception):
    pass


def test_python_rules_raise_without_a_device(monkeypatch):
    """Every PcmError of the stretch arguments is raised before the library loads; good arguments reach it; with both None the
    call is the one without the arguments."""
    from parseoggvorbis_amd import pcm

    def no_load():
        raise AssertionError("library loaded before the arguments were checked")

    def reached():
        raise _Reached()
    monkeypatch.setattr(pcm, "_load", no_load)
    two = [b"OggS", b"OggS"]
    for word, kw in [("mono=True", dict(time_stretch=1.1, mono=False)), ("mono=True", dict(pitch_shift=1, sr=16000, mono=False)),
                     ("sr=", dict(pitch_shift=1)), ("exclude", dict(time_stretch=1.1, pitch_shift=1, sr=16000)),
                     ("hpss", dict(time_stretch=1.1, hpss="harmonic")), ("hpss", dict(pitch_shift=1, sr=16000, hpss="percussive")),
                     ("time_stretch", dict(time_stretch=0.0)), ("time_stretch", dict(time_stretch=-1.0)),
                     ("time_stretch", dict(time_stretch=float("nan"))), ("time_stretch", dict(time_stretch=float("inf"))),
                     ("time_stretch", dict(time_stretch=[1.0, 0.0])), ("2 files", dict(time_stretch=[1.0])),
                     ("2 files", dict(time_stretch=[1.0, 1.0, 1.0])), ("2 files", dict(pitch_shift=[1.0], sr=16000)),
                     ("time_stretch", dict(time_stretch="fast")), ("time_stretch", dict(time_stretch=True)),
                     ("pitch_shift", dict(pitch_shift=float("nan"), sr=16000)), ("pitch_shift", dict(pitch_shift=[1, float("inf")], sr=16000)),
                     ("pitch_bins_per_octave", dict(pitch_shift=1, sr=16000, pitch_bins_per_octave=0)),
                     ("above the limit", dict(pitch_shift=7, sr=96000)),
                     ("stretch_n_fft", dict(time_stretch=1.1, stretch_n_fft=1000)), ("stretch_n_fft", dict(time_stretch=1.1, stretch_n_fft=8)),
                     ("stretch_hop_length", dict(time_stretch=1.1, stretch_hop_length=0)),
                     ("stretch_win_length", dict(time_stretch=1.1, stretch_win_length=4096))]:
        kw.setdefault("mono", True)
        with pytest.raises(pcm.PcmError) as ei:
            pcm.get_pcm_batch(two, **kw)
        assert word in str(ei.value), (word, str(ei.value))
    with pytest.raises(pcm.PcmError):
        pcm.get_pcm_from_raw_bytes(b"OggS", mono=True, time_stretch=[1.0, 2.0])
    monkeypatch.setattr(pcm, "_load", reached)
    for kw in (dict(time_stretch=0.8), dict(time_stretch=[0.9, 1.1]), dict(time_stretch=np.float32(1.5), trim_db=40.0, loudness_normalize=-23.0),
               dict(pitch_shift=[3, -2], sr=22050), dict(pitch_shift=-1.5, sr=16000, pitch_bins_per_octave=24, stretch_n_fft=512, stretch_hop_length=100,
                                                         stretch_win_length=400),
               dict(time_stretch=None, pitch_shift=None, stretch_n_fft=7)):  # off: its other arguments are not looked at
        with pytest.raises(_Reached):
            pcm.get_pcm_batch(two, mono=True, **kw)
    spec, r, hz = pcm.stretch_args(2, pitch_shift=[12, -12], sr=16000)
    assert (spec.n_fft, spec.hop_length, spec.win_length, spec.options, spec.shift_to_hz) == (2048, 512, 2048, 1, 16000)
    assert list(r) == [0.5, 2.0] and list(hz) == [32000, 8000]
    spec, r, hz = pcm.stretch_args(3, time_stretch=1.25, stretch_n_fft=256)
    assert (spec.n_fft, spec.hop_length, spec.options, spec.shift_to_hz, hz) == (256, 64, 0, 0, None) and list(r) == [1.25] * 3
