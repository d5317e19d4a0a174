"""The pyin kernels (csrc/vsyn_pyin.h) where B, N and the trough count leave one stride of a thread loop, on the cases of
tests/pyin_regime_cases.py, against the float64 model of tests/pyin_model.py: decode for vsyn_pyin_decode_device, pyin for
vsyn_pyin_device. tests/test_pyin_regimes_cpu.py asserts that every case is decided and reaches its branch.

The gates are those of tests/test_gpu_pyin.py, derived in the model and not tuned on the device: states equal on EVERY frame and the
path's score within 2 E[-1] of the model's optimum; the voiced flag and the bin equal, f0 equal bit for bit,
|d vp| <= (2^-24 + pbound + 4096 * 2^-53) * vp."""
import numpy as np
import pytest

from tests import pyin_regime_cases as rc
from tests.test_gpu_condition import blobs, mods, pcm_by_rate, synth  # noqa: F401
from tests.test_gpu_pyin import _check_path, _check_rows, _decode, _run
from tests.test_gpu_trim import VARIANTS, _batch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(rc.DECODE))
def test_decode_alone_in_every_regime(synth, name):
    """vsyn_pyin_decode_device on the crafted rows of the regime, all its segments in one launch (two rates: two widths), and once
    more in reverse order."""
    r = rc.DECODE[name]
    segs, mods_ = rc.decode_segments(name), rc.decode_models(name)
    spec = rc.spec(r)
    got = _decode(synth, spec, [s["sr"] for s in segs], [s["obs"] for s in segs])
    for s, m, st in zip(segs, mods_, got):
        assert st.shape[0] == s["obs"].shape[0]
        _check_path(st, m, (name, s["kind"], s["arg"], s["sr"]))
    back = _decode(synth, spec, [s["sr"] for s in segs][::-1], [s["obs"] for s in segs][::-1])
    for s, m, st in zip(segs[::-1], mods_[::-1], back):
        assert np.array_equal(st, m["states"]), (name, s["kind"], s["arg"], "reversed")


@pytest.mark.parametrize("group", list(rc.STAGE))
def test_the_stage_in_every_regime_of_the_observation_kernel(synth, group):
    """vsyn_pyin_device on every case of the group, one launch per channel count, the stride / offset variants of the trim stage's
    test in rotation. Prints the worst |d vp| / bound."""
    cases, models = rc.stage_group(group), rc.stage_models(group)
    spec = rc.spec(rc.STAGE[group])
    worst = 0.0
    for k, Cn in enumerate((1, 2, 3)):
        sub = [i for i, c in enumerate(cases) if c["C"] == Cn]
        if not sub:
            continue
        odd, in_off, _ = VARIANTS[(k + list(rc.STAGE).index(group)) % len(VARIANTS)]
        x, frames = _batch([cases[i]["x"] for i in sub], odd)
        rates = [cases[i]["sr"] for i in sub]
        got = _run(synth, spec, x, frames, rates, in_off)
        assert not got["refused"].any()
        for j, i in enumerate(sub):
            worst = max(worst, _check_rows(got["rows"][j], models[i], cases[i], (group, Cn, cases[i]["kind"], frames[j], rates[j])))
    print("pyin regimes (%s): worst |d vp| / bound %.4f" % (group, worst))


def test_2049_bins_are_refused_with_nothing_launched(synth):
    """B = 2049 is one state pair above the cap: VSYN_ERR_INVALID from the stage and the decode entry, and nothing is written."""
    import torch
    from parseoggvorbis_amd import pitch
    from parseoggvorbis_amd.binding import VsynError
    spec = pitch.pyin_spec(rc.C2, rc.FMAX_2048, 2048, 512, resolution=0.03)
    spec.fmax = rc.FMAX_2049
    t = torch.full((256,), 5.0, dtype=torch.float32, device="cuda")
    f = torch.full((8,), 64, dtype=torch.int32, device="cuda")
    o = torch.full((64,), 9, dtype=torch.int32, device="cuda")
    d = torch.full((2 * 2049,), 0.25 / 2049, dtype=torch.float64, device="cuda")
    with pytest.raises(VsynError) as ei:
        synth.pyin_device(spec, [22050], t.data_ptr(), 64, 2, f.data_ptr(), t.data_ptr() + 512, o.data_ptr(), o.data_ptr() + 32)
    assert ei.value.code == 1, str(ei.value)
    with pytest.raises(VsynError) as ei:
        synth.pyin_decode_device(spec, [22050], d.data_ptr(), [2], o.data_ptr())
    assert ei.value.code == 1, str(ei.value)
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == 5.0).all() and (o.cpu().numpy() == 9).all()
