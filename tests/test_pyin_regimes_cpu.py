"""The cases of tests/pyin_regime_cases.py on the CPU, from the model alone (tests/pyin_model.py): every decision of every one of
them is decided (the allowed share of undecided cases and frames is zero), so that tests/test_gpu_pyin_regimes.py may ask for equal
states on every frame, and every case reaches the stride, wave, clamp or branch of csrc/vsyn_pyin.h that it is there for."""
import ctypes

import numpy as np
import pytest

from parseoggvorbis_amd import pitch
from tests import pyin_model as ym
from tests import pyin_regime_cases as rc


def _h(s):
    return s["w"] // 2


def _jumps(s, m):
    """|difference of the bins| of consecutive frames of the optimal path."""
    return np.abs(np.diff(m["states"] % s["B"]))


@pytest.mark.parametrize("name", list(rc.DECODE))
def test_every_decode_regime_has_its_sizes_and_is_decided(name):
    r = rc.DECODE[name]
    bps, B = ym.num_bins(r["fmin"], r["fmax"], r["resolution"])
    assert tuple((B, ym.width(sr, r["H"], r["mtr"], bps)) for sr in r["rates"]) == r["BW"]
    assert 2 * B <= 4096 and all(w % 2 == 1 for _, w in r["BW"])
    for s, m in zip(rc.decode_segments(name), rc.decode_models(name)):
        bad = [x for x in m["margins"] if not x[1] > x[2]]
        assert m["decided"] and not bad, (name, s["kind"], s["arg"], bad[:3])
        assert (s["obs"] >= 0).all() and (s["obs"].sum(axis=1) <= 1.0 + 1e-15).all()
        assert len(m["states"]) == s["obs"].shape[0] and (1 <= s["obs"].shape[0] <= 8 or s["kind"] == "long")
    if name in rc.LARGE:
        assert all(s["obs"].shape[0] <= 6 for s in rc.decode_segments(name))


def test_the_sizes_are_the_ones_the_kernel_branches_on():
    BW = {n: r["BW"][0] for n, r in rc.DECODE.items()}
    assert BW["stride2"] == (1201, 201) and 2 * 1024 < 2 * 1201 <= 3 * 1024 and -(-1201 // 128) == 10  # q = 2; 10 waves with an element
    assert BW["stride3"] == (2048, 341) and 2 * 2048 == 4 * 1024 and 2048 // 128 == 16               # q = 3; all 16 waves
    assert BW["h0_few"] == (12, 1) and BW["h0_many"] == (601, 1) and rc.DECODE["h0_few"]["BW"][1] == (12, 3)
    for n in ("no_oob", "b_h1"):
        B, w = BW[n]
        assert B <= w // 2 + 1  # oob == false
    assert BW["no_oob"] == (59, 141) and BW["b_h1"] == (36, 71) and BW["b_h2"] == (37, 71) and 37 == 71 // 2 + 2
    assert [BW[n] for n in ("b_wm1", "b_w", "b_wp1")] == [(70, 71), (71, 71), (72, 71)]
    assert BW["long"] == (12, 3) and sorted(s["obs"].shape[0] for s in rc.decode_segments("long"))[::2] == [1, 1100]
    assert rc.DECODE["sw03"]["sw"] == 0.3 and rc.DECODE["sw049"]["sw"] == 0.49 and rc.DECODE["h0_many"]["mtr"] == 1.0
    assert ym.num_bins(rc.C2, rc.FMAX_2049, 0.03) == (34, 2049)
    for n in ("stride2", "h0_few", "b_wp1", "sw03"):  # two widths in one launch
        assert len({w for _, w in rc.DECODE[n]["BW"]}) == 2


@pytest.mark.parametrize("name", list(rc.DECODE))
def test_every_decode_regime_reaches_its_branch(name):
    segs, mods = rc.decode_segments(name), rc.decode_models(name)
    B0, w0 = rc.DECODE[name]["BW"][0]
    out = [(s, m, np.flatnonzero(_jumps(s, m) > _h(s))) for s, m in zip(segs, mods)]
    if B0 > w0 // 2 + 1:  # a back pointer on the optimal path is a source outside the band
        assert any(len(j) for _, _, j in out)
    else:  # every source lies in the band
        assert all(len(j) == 0 for _, _, j in out)
    if name == "b_h2":  # the only targets with such a source are 0 and B - 1, from B - 1 and 0
        js = [(m["states"][t] % B0, m["states"][t + 1] % B0) for s, m, j in out for t in j]
        assert js and set(js) <= {(0, B0 - 1), (B0 - 1, 0)} and len(set(js)) == 2
    if name in rc.LARGE:
        top = 3072 if name == "stride3" else 2048
        assert any((m["states"] >= top).any() for m in mods)
        # and as the SOURCE of a jump out of the band (the 2-byte scan states and the back pointer hold it)
        assert any(m["states"][t] >= top for s, m, j in out for t in j)
        assert max(int(m["states"].max()) for m in mods) == 2 * B0 - 1
    if name in rc.H0:
        for s, m in zip(segs, mods):
            if s["w"] == 1 and s["kind"] in ("alternate", "up", "down"):  # (an unvoiced state cannot move at all: its band is itself)
                assert (np.diff(m["states"]) != 0).any(), (name, s["kind"])
        assert sum(s["w"] == 1 and s["kind"] in ("alternate", "up", "down") for s in segs) >= 3
    for s, m in zip(segs, mods):
        B, h, st = s["B"], _h(s), list(m["states"])
        nz = [np.flatnonzero(r) for r in s["obs"]]
        if s["kind"] in ("alternate", "up", "down", "up_far", "down_far"):
            assert st == [int(b[0]) for b in nz], (name, s["kind"], st)
        if s["kind"] == "alternate":
            assert st == [0, B - 1, B - 1, 0]
        if s["kind"] in ("up", "down"):  # the source is the last element of the prefix, or the first of the suffix
            assert st[0] == s["arg"] and st[1] - st[0] == (h + 1 if s["kind"] == "up" else -h - 1)
        if s["kind"] in ("up_far", "down_far"):  # the looked-up element lies in the wave next to the source's
            e = st[1] - h - 1 if s["kind"] == "up_far" else st[1] + h + 1
            assert st[0] == s["arg"] and e // 128 - st[0] // 128 == (1 if s["kind"] == "up_far" else -1), (name, st)
        if s["kind"] in ("tie_hi", "tie_lo", "tie_hi_far", "tie_lo_far"):  # the lower of two sources that tie in every bit
            a, b = nz[0]
            d = h + 1 + (rc.TIE_FAR if s["kind"].endswith("far") else 0)
            to = b + d if s["kind"].startswith("tie_hi") else a - d
            assert b == a + 1 and st == [a, to], (name, st)
            assert m["log_obs"][0][a] == m["log_obs"][0][b] and (B <= 256 or a // 128 != b // 128)
        if s["kind"] == "pair":
            a = nz[0][0]
            assert st == [a] * len(st) and nz[0][1] == B - 1 - a
        if s["kind"] == "vtie":  # voiced i against all B unvoiced states, every stride of the arg-max: i wins
            i = nz[0][0]
            lo = m["log_obs"][0]
            assert st == [i] and (lo[B:] == lo[i]).all() and (lo[:B] == lo[i]).sum() == 1
        if s["kind"] == "unv_hi":
            assert st[:3] == [B - 1, 2 * B - 1, h + 1] and st[1] - B - st[2] > h, (name, st)
        if s["kind"] == "unv_lo":
            assert st[:3] == [0, B, B - 2 - h], (name, st)
        if s["kind"] == "unv_end":  # the final arg-max lies in the last stride
            assert st == [B - 1, 2 * B - 1] and (2 * B - 1) // 1024 == (3 if name == "stride3" else 2), (name, st)
    if name == "long":
        big = [m for m in mods if len(m["states"]) == 1100][0]
        j = np.flatnonzero(np.abs(np.diff(big["states"] % B0)) > 1)
        assert len(set(big["states"])) >= 8 and len(j) >= 25 and (j > 1024).any()  # jumps out of the band, behind frame 1024 too
    kinds = {s["kind"] for s in segs}
    if name == "stride2":
        assert {"up", "down", "tie_hi_far", "tie_lo_far"} <= kinds
    if name in rc.LARGE:
        assert {"sparse", "alternate", "up_far", "down_far", "tie_hi", "tie_lo", "vtie", "unv_hi", "unv_end"} <= kinds
        ms = [s["arg"] for s in segs if s["kind"] in ("up", "down", "up_far", "down_far", "tie_hi", "tie_lo", "tie_hi_far", "tie_lo_far")]
        assert all(x % 128 in (0, 127) for x in ms) and any(x >= 1024 for x in ms)  # a wave's first or last element; above bin 1024


# ---- the library's host-only entry: the specs pass its checks, and the cap of the states ----

def _transition(spec, sr):
    from parseoggvorbis_amd import binding
    lib = binding.load()
    w, B, err = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_char_p()
    rc_ = lib.vsyn_pyin_transition(ctypes.byref(spec), sr, ctypes.byref(w), ctypes.byref(B), None, 0, ctypes.byref(err))
    return rc_, B.value, w.value, err.value


def test_every_spec_passes_the_librarys_checks_with_the_models_sizes():
    for name, r in rc.DECODE.items():
        for sr, bw in zip(r["rates"], r["BW"]):
            assert _transition(rc.spec(r), sr)[:3] == (0,) + bw, (name, sr)
    for group in rc.STAGE:
        for c, m in zip(rc.stage_group(group), rc.stage_models(group)):
            assert _transition(rc.spec(c), c["sr"])[:3] == (0, m["B"], m["w"]), (group, c["sr"])


def test_2048_bins_are_accepted_and_2049_refused():
    from parseoggvorbis_amd import binding
    lib = binding.load()
    err = ctypes.c_char_p()
    w, B = ctypes.c_uint32(0), ctypes.c_uint32(0)
    ok = pitch.pyin_spec(rc.C2, rc.FMAX_2048, 2048, 512, resolution=0.03)
    assert lib.vsyn_pyin_transition(ctypes.byref(ok), 22050, ctypes.byref(w), ctypes.byref(B), None, 0, ctypes.byref(err)) == 0
    assert (B.value, w.value) == (2048, 341) and lib.vsyn_pyin_num_bins(ctypes.byref(ok)) == 2048
    with pytest.raises(pitch.PyinError):
        pitch.pyin_spec(rc.C2, rc.FMAX_2049, 2048, 512, resolution=0.03)
    bad = pitch.pyin_spec(rc.C2, rc.FMAX_2048, 2048, 512, resolution=0.03)
    bad.fmax = rc.FMAX_2049
    assert lib.vsyn_pyin_transition(ctypes.byref(bad), 22050, None, None, None, 0, ctypes.byref(err)) == 1 and b"states" in err.value
    assert lib.vsyn_pyin_num_bins(ctypes.byref(bad)) == 0


# ---- B. the observation kernel's cases ----

@pytest.mark.parametrize("group", list(rc.STAGE))
def test_every_stage_case_is_decided(group):
    for c, m in zip(rc.stage_group(group), rc.stage_models(group)):
        bad = [x for x in m["margins"] if not x[2] > x[3]]
        assert m["decided"] and not bad, (group, c["kind"], c["sr"], bad[:3])
        assert m["dec"]["decided"], (group, c["kind"], [x for x in m["dec"]["margins"] if not x[1] > x[2]][:3])
        assert len(m["states"]) >= 9 and not m["refused"]


def _troughs(m):
    return [len(f["lags"]) for f in m["frames"]]


def test_the_threshold_counts_fill_and_overfill_the_tile():
    assert [rc.tile_rows(N) for N in (1, 100, 256, 257, 1024)] == [64, 30, 11, 11, 2]
    for group, N in (("n1", 1), ("n256", 256), ("n257", 257), ("n1024", 1024)):
        TR = rc.tile_rows(N)
        cs, ms = rc.stage_group(group), rc.stage_models(group)
        assert all(c["N"] == N and rc.beta(N).shape == (N,) for c in cs)
        K = [k for m in ms for k in _troughs(m)]
        assert any(0 < k <= TR for k in K), (group, sorted(set(K)))
        if N >= 256:
            assert any(k > TR for k in K) and any(k > 2 * TR for k in K), (group, sorted(set(K)))  # a second and a third tile
        assert any(m["voiced"].any() for m in ms) and any((~m["voiced"]).any() for m in ms)
        assert {c["C"] for c in cs} == {1, 2, 3} and {c["sr"] for c in cs} == {8000, 16000}
        assert {m["p_max"] - m["p_min"] + 1 for m in ms} == {61, 121}


def test_the_trough_counts_leave_one_stride_and_two():
    K410 = [max(_troughs(m)) for m in rc.stage_models("k410")]
    assert all(256 < k <= 512 for k in K410), K410
    assert sum(int(m["voiced"].sum()) for m in rc.stage_models("k410")) >= 9
    K690 = [max(_troughs(m)) for m in rc.stage_models("k690")]
    assert all(k > 512 for k in K690), K690
    m = rc.stage_models("k_coarse")[0]
    assert m["bps"] == 2 and max(_troughs(m)) > 256
    crossing = 0
    for f in m["frames"]:
        cand = np.flatnonzero((f["P"] > 0) & (f["bins"] >= 0) & (f["bins"] < m["B"]))
        lo, hi = cand[cand < 256], cand[cand >= 256]
        if len(lo) and len(hi) and f["bins"][lo[-1]] == f["bins"][hi[0]]:  # k < 256 <= k2, neighbours among the candidates, one bin
            crossing += 1
    assert crossing >= 1
    # the minimum, its first index and a winner all lie beyond the first stride somewhere
    for group in ("k410", "k690"):
        fr = [f for m in rc.stage_models(group) for f in m["frames"] if len(f["lags"]) > 256]
        assert any(int(np.argmin(f["h"])) >= 256 for f in fr) and any((f["P"][256:] > 0).any() for f in fr), group
    assert {c["C"] for g in ("k410", "k690", "k_coarse") for c in rc.stage_group(g)} == {1, 2, 3}


def test_the_parameters_are_not_the_defaults():
    for group, lam, ntp in (("lam05", 0.5, 0.0), ("lam8", 8.0, 1.0)):
        cs, ms = rc.stage_group(group), rc.stage_models(group)
        assert all((c["lam"], c["ntp"]) == (lam, ntp) and c["lam"] >= 0.5 for c in cs)
        assert all(m["voiced"].sum() >= 5 and len(set(m["bins"][m["voiced"]])) >= 2 for m in ms)  # both steps of the tone are decoded
        assert any(len(f["lags"]) >= 2 and (f["P"] > 0).sum() >= 2 for m in ms for f in m["frames"])  # the prior has more than one position
        assert {c["sr"] for c in cs} == {8000, 16000}
