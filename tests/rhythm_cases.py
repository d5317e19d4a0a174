"""Inputs shared by tests/test_rhythm_cpu.py (which asserts that each one decides its comparisons by more than the band two float64
evaluations can disagree in) and tests/test_gpu_rhythm.py (which runs them on the device)."""
import numpy as np

from tests import rhythm_model as rm

# rate = hop = 1: a time in seconds is its count of frames, so the windows below are frames
FRAMES = dict(rate=1, hop=1)


def _plateaus(F, seed):
    r = np.random.default_rng(seed)
    return (np.round(r.random(F) * 4.0) / 4.0).astype(np.float32)


def _spikes(F, at):
    x = np.full(F, 0.25, np.float32)
    x[[a for a in at if a < F]] = 1.0
    return x


def peak_cases():
    """(name, envelope, rate, hop, times dict, delta, normalize)"""
    out = []
    for F in (1, 63, 64, 65, 4097):
        x = rm.envelope(F, 100 + F)
        for wait in (0, 1, min(F + 1, 4096)):
            t = dict(pre_max=1, post_max=0, pre_avg=4, post_avg=4, wait=wait)
            out.append(("F%d_wait%d" % (F, wait), x, 1, 1, t, 0.07, True))
        out.append(("F%d_wide" % F, x, 1, 1, dict(pre_max=4096, post_max=4095, pre_avg=4096, post_avg=4095, wait=2), 0.01, True))
        out.append(("F%d_raw" % F, x, 1, 1, dict(pre_max=2, post_max=1, pre_avg=3, post_avg=2, wait=1), 0.07, False))
        out.append(("F%d_plateaus" % F, _plateaus(F, 7 + F), 1, 1, dict(pre_max=2, post_max=2, pre_avg=3, post_avg=3, wait=0), 0.07, True))
    for wait in (0, 1):
        t = dict(pre_max=1, post_max=0, pre_avg=2, post_avg=2, wait=wait)
        out.append(("boundary_wait%d" % wait, _spikes(200, (62, 63, 64, 65, 127, 128, 191, 192)), 1, 1, t, 0.07, True))
    for delta in (0.0, 0.07):
        out.append(("constant_delta%g" % delta, np.full(130, 0.5, np.float32), 22050, 512, dict(rm.PEAK_TIMES), delta, True))
        out.append(("zeros_delta%g" % delta, np.zeros(70, np.float32), 22050, 512, dict(rm.PEAK_TIMES), delta, True))
    out.append(("clicks_22050", rm.click_train(), 22050, 512, dict(rm.PEAK_TIMES), 0.07, True))
    out.append(("clicks_44100", rm.click_train(period=37, first=11), 44100, 512, dict(rm.PEAK_TIMES), 0.07, True))
    out.append(("negative", rm.envelope(300, 5, negative=True), 16000, 160, dict(rm.PEAK_TIMES), 0.07, True))
    return out


def tempo_cases():
    """(name, envelope, rate, hop, W, tempo arguments)"""
    return [
        ("clicks20", rm.click_train(), 22050, 512, 384, {}),
        ("clicks20_ac8", rm.click_train(), 22050, 512, 344, {}),
        ("clicks37", rm.click_train(F=900, period=37, first=11), 44100, 512, 689, {}),
        ("clicks9_fast", rm.click_train(F=400, period=9, first=2), 22050, 512, 128, dict(start_bpm=240.0, std_bpm=0.5, max_tempo=None)),
        ("clicks50_slow", rm.click_train(F=800, period=50, first=0), 22050, 512, 384, dict(start_bpm=60.0, max_tempo=100.0)),
    ]
