"""The tuning kernels (csrc/vsyn_tuning.h) on frames built to hold chosen peaks: the cases of tests/tuning_reduction_cases.py, which
tests/test_tuning_reduction_cpu.py certifies from the model alone. Everything here is exact; there is no tolerance.

Each launch of a group runs as one call that holds all its segments, and again with the segments reversed; results follow their
segment. Per segment:
  the dense rows of vsyn_piptrack_device equal tuning_model.piptrack on the device's own lin_power rows, bit for bit (in group D the
  linear kernel's 8 frames a workgroup against piptrack's 1);
  vsyn_tuning_device's counts equal (n, selected) of tuning_model.pitch_tuning on the device's dense rows, its tuning equals the single
  admitted value, and both equal binding.pitch_tuning (the host reduction) on those rows;
  what the case claims holds on the device's rows (check_claims of the CPU module), and the classes reached are asserted per group:
  the middle pair splits in the top byte, byte 2, byte 1 and byte 0 and all magnitudes are equal (A); ties of two and three bins, in
  either order of their threads and within one thread's stride, and the winner in bin 0 and bin nbin - 1 (B); the fullest frame at
  cap (C); tile 1 (D).
Each test prints one line: launches, segments, records, and the classes reached."""
import ctypes as C

import numpy as np
import pytest

from tests import tuning_model as tm
from tests import tuning_reduction_cases as rc
from tests.test_gpu_tuning import batch, mods, run_lin_power, run_piptrack, run_tuning, same_bits, synth  # noqa: F401
from tests.test_tuning_reduction_cpu import check_claims

pytestmark = pytest.mark.gpu


def run_launch(synth, tuning, L, reached):
    """One launch forwards and reversed; returns the records counted."""
    from parseoggvorbis_amd import binding
    p = rc.params(L)
    n = L["n_fft"]
    spec = tuning.framing_spec(n, L["hop"], L["win"], L["center"], L["power"])
    tun = tuning.tuning_spec(**L["tun"])
    records = 0
    for order in ("forwards", "reversed"):
        segs = L["segs"] if order == "forwards" else L["segs"][::-1]
        pcm, frames = batch([s["y"] for s in segs])
        rates = [s["sr"] for s in segs]
        rows = run_piptrack(synth, spec, tun, pcm, frames, rates)
        lin = run_lin_power(synth, spec, pcm, frames, rates)
        t, c = run_tuning(synth, spec, tun, pcm, frames, rates)
        for i, s in enumerate(segs):
            what = (L["name"], s["name"], order)
            pitch, mag = rows[i]
            wp, wm = tm.piptrack(lin[i], s["sr"], n, p["fmin"], p["fmax"], p["threshold"])
            assert same_bits(pitch, wp) and same_bits(mag, wm), what
            want = check_claims(L, s, pitch, mag, reached, what)  # (one admitted tuning among them)
            assert (int(c[i, 0]), int(c[i, 1])) == (want["n"], want["selected"]), (what, c[i], want)
            assert t[i] == want["tuning"], (what, t[i], want)
            assert binding.pitch_tuning(pitch, mag, p["resolution"], p["bins_per_octave"]) == (float(t[i]), int(c[i, 0]), int(c[i, 1])), what
            if s["frames"] is not None:  # the crafted tones inside the band are the peaks, and nothing else is
                k_lo, k_hi = tm.bins(s["sr"], n, p["fmin"], p["fmax"])
                counts = [sum(k_lo <= k < k_hi for k, _ in tones) for tones in s["frames"][:pitch.shape[0]]]
                assert rc.per_frame(pitch).tolist() == counts, what
            if order == "forwards":
                records += want["n"]
    return records


def run_group(mods, synth, group):
    _, tuning = mods
    reached = set()
    records = sum(run_launch(synth, tuning, L, reached) for L in rc.launches()[group])
    Ls = rc.launches()[group]
    print("tuning reduction (%s): %d launches, %d segments, %d records; reached: %s" %
          (group, len(Ls), sum(len(L["segs"]) for L in Ls), records, sorted(reached, key=str)))
    return reached


def test_the_selection_in_every_byte_of_the_key(mods, synth):
    reached = run_group(mods, synth, "select")
    assert {("klass", 3), ("klass", 2), ("klass", 1), ("klass", 0), ("klass", "equal"), ("klass", "odd")} <= reached, reached


def test_the_first_arg_max_on_ties_and_at_both_ends(mods, synth):
    reached = run_group(mods, synth, "hist")
    assert {("tied", 1), ("tied", 2), ("tied", 3), ("bin", "first"), ("bin", "last"), ("far", "first thread lower"), ("far", "first thread higher"),
            ("far", "same thread")} <= reached, reached


def test_the_compaction_at_exactly_cap_records_a_frame(mods, synth):
    reached = run_group(mods, synth, "cap")
    assert {("cap", 45), ("cap", 127), ("cap", 14)} <= reached, reached


def test_one_frame_a_workgroup_on_the_direct_path(mods, synth):
    _, tuning = mods
    for n, hop, center in rc.TILE1:
        assert synth.lib.vsyn_piptrack_tile(C.byref(tuning.framing_spec(n, hop, n, center))) == 1
    reached = run_group(mods, synth, "tile1")
    print("tuning reduction (tile1): vsyn_piptrack_tile 1 at %s" % (rc.TILE1,))
    assert reached


def test_segments_without_a_frame_or_a_peak_between_crafted_ones(mods, synth):
    reached = run_group(mods, synth, "empty")
    assert ("klass", "none") in reached and ("klass", "odd") in reached, reached
