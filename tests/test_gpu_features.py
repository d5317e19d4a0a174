"""Feature matrices on the GPU (vsyn_features_*, ogg_vorbis_features_corpus, parseoggvorbis_amd/features.py) against the
reference's own matrices (tests/golden/features_*.npz, made by tools/make_feature_goldens.py): floor kinds bit for bit,
residue kinds within 2 ulp (numpy's log1pf / expf against the device's)."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = ["test.stereo44khz", "test.mono44khz"] + ["synth_%02d" % i for i in range(16)] + ["winflags_bcd"]

pytestmark = pytest.mark.gpu


def _ogg(name):
    return open(os.path.join(GOLDEN, name + ".ogg"), "rb").read()


def _golden(name):
    z = np.load(os.path.join(GOLDEN, "features_%s.npz" % name))
    return json.loads(str(z["grid"])), z


# Largest difference seen between the device and the reference's numpy on the golden grid, in ulp of the row value: 0 for the floor
# kinds and for residue rows without the exp factor, 3 for residue_ys_with_floor without log1p_abs_space (one element of synth_02).
# There the row is x * exp(floor_base - 1): numpy's float32 exp is up to 1.8 ulp from the exact value on these arguments while the
# device rounds once from double, and the product carries that relative error into the larger row value. Bound: 4 ulp there, 2
# elsewhere.
def assert_close(got, want, kind, what, kw=None):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if kind.startswith("floor"):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what
    else:
        k = 4 if kind == "residue_ys_with_floor" and not (kw or {}).get("log1p_abs_space") else 2
        tol = k * np.spacing(np.maximum(np.abs(got), np.abs(want)))
        bad = np.abs(got.astype(np.float64) - want) > tol
        assert not bad.any(), (what, np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


@pytest.fixture(scope="module")
def feats():
    import torch
    assert torch.cuda.is_available()
    from parseoggvorbis_amd import features
    return features


def test_every_fixture_and_grid_entry_equals_the_reference(feats):
    grid, _ = _golden(FILES[0])
    datas = [_ogg(n) for n in FILES]
    gz = {n: _golden(n)[1] for n in FILES}
    for i, (kind, dim, kw) in enumerate(grid):
        res = feats.get_features_batch(datas, dim, kind, errors="return", **kw)
        for name, got in zip(FILES, res):
            z = gz[name]
            what = (name, i, kind, dim, kw)
            if "e%d" % i in z.files:
                assert isinstance(got, feats.FeatureError), what
                assert "feature-index" in str(got), (what, str(got))
            else:
                assert not isinstance(got, Exception), (what, str(got))
                assert_close(got, z["c%d" % i], kind, what, kw)


@pytest.mark.parametrize("name", ["test.stereo44khz", "synth_05"])
def test_drop_in_interface(feats, name):
    grid, z = _golden(name)
    lib = feats.ParseOggVorbisLib.get_instance()
    for i in (0, 4, 13):
        kind, dim, kw = grid[i]
        assert_close(lib.get_features_from_raw_bytes(_ogg(name), dim, kind=kind, **kw), z["c%d" % i], kind, (name, i), kw)


def test_output_dim_below_the_biggest_floor_is_refused_for_residue_kinds(feats):
    with pytest.raises(feats.FeatureError) as ei:
        feats.get_features_from_raw_bytes(_ogg("test.stereo44khz"), 10, kind="residue_ys")  # 29 posts
    assert "below the biggest floor" in str(ei.value)


def _submits(feats, datas, entry):
    """GPU submits of one corpus run (one feeder, three files per submit): the run's statistics, from the corpus call itself."""
    import ctypes as C
    from parseoggvorbis_amd import _corpus
    kind, dim, kw = entry
    spec, lib, stats = feats.feature_spec(dim, kind, **kw), feats._load(), []
    counts = np.zeros(len(datas), np.uint64)
    _corpus.run(lib, lib.ogg_vorbis_features_corpus, datas, (4, 1, 3, 0, C.byref(spec)), (counts,), lambda i, p: None, feats.FeatureError,
                "return", "features", stats)
    return stats[5]


@pytest.mark.parametrize("feeders", [1, 3])
def test_corpus_replicated_with_a_damaged_file(feats, feeders):
    """A replicated corpus with one damaged file (file 7: a page checksum broken half way). Grid entry 15 is refused on the device
    for synth_04 and synth_11 (feature-index, as the reference raises): their replicas share a setup each, so with one feeder
    their submits of three are flagged and re-run file by file, and each replica fails alone."""
    names = ["test.stereo44khz", "synth_03", "test.mono44khz", "winflags_bcd", "synth_04", "synth_11"] * 3
    datas = [_ogg(n) for n in names]
    bad = bytearray(datas[7])
    bad[len(bad) // 2:len(bad) // 2 + 64] = bytes(64)  # breaks a page checksum half way
    datas[7] = bytes(bad)
    grid, _ = _golden(names[0])
    if feeders == 1:  # entry 15 re-runs the two flagged submits of three file by file: six submits more than entry 14
        assert _submits(feats, datas, grid[15]) - _submits(feats, datas, grid[14]) == 6
    for i in (1, 7, 14, 15):
        kind, dim, kw = grid[i]
        res = feats.get_features_batch(datas, dim, kind, threads=4, feeders=feeders, files_per_submit=3, errors="return", **kw)
        for j, (name, got) in enumerate(zip(names, res)):
            z = _golden(name)[1]
            if j == 7:
                assert isinstance(got, feats.FeatureError) and "file 7" in str(got), str(got)
            elif "e%d" % i in z.files:
                assert isinstance(got, feats.FeatureError) and "feature-index" in str(got), (j, name, i, str(got))
            else:
                assert_close(got, z["c%d" % i], kind, (j, name, i), kw)


def test_features_between_submits_leave_the_pcm_alone(feats):
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec, synth_batch
    spec = fixture_like_spec(2)
    b1 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=3)
    b2 = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=4)
    seg2 = b2["segments"].copy()
    seg2["flags"] = 0  # continue the streams of b1
    runs = []
    for with_features in (False, True):
        s = Synth(spec, device=0, max_streams=4)
        r1 = s.submit_host(b1["packets"], b1["segments"], b1["ys"], b1["residue"], b1["plane_stride"])
        if with_features:
            for kind, dim, kw in (("floor_final_ys_rendered", 40, {}), ("residue_ys_with_floor", 70, {"log1p_abs_space": True})):
                f = s.features_host(feats.feature_spec(dim, kind, **kw), b2["packets"], b2["segments"], b2["ys"], b2["residue"])
                assert f["rc"] == 0 and f["rows"].shape[0] > 0
        r2 = s.submit_host(b2["packets"], seg2, b2["ys"], b2["residue"], b2["plane_stride"])
        assert r1["rc"] == 0 and r2["rc"] == 0
        runs.append((r1["pcm"], r2["pcm"], r2["emit_len"]))
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def test_segments_with_and_without_rows(feats):
    """vsyn_features_host over several segments: each segment's rows equal its rows alone; a segment of packets without a used
    floor yields none."""
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec, synth_batch
    spec = fixture_like_spec(2)
    b = synth_batch(spec, streams=4, packets_per_stream=10, pattern="mixed", seed=11)
    pk = b["packets"].copy()
    seg = b["segments"]
    g = seg[2]
    pk["floor_used"][g["first_packet"]:g["first_packet"] + g["num_packets"]] = 0
    s = Synth(spec, device=0, max_streams=4)
    fs = feats.feature_spec(20, "floor_final_ys")
    whole = s.features_host(fs, pk, seg, b["ys"], b["residue"])
    assert whole["rc"] == 0 and whole["seg_rows"][2] == 0 and whole["seg_rows"][0] > 0
    off = np.concatenate([[0], np.cumsum(whole["seg_rows"])]).astype(int)
    for k in range(len(seg)):
        one = s.features_host(fs, pk, seg[k:k + 1], b["ys"], b["residue"])
        assert np.array_equal(one["rows"], whole["rows"][off[k]:off[k + 1]])



# ---- randomised batches against the independent model (tests/feature_model.py, fed by the CPU oracle's taps) ----

def _xs(rng, n2, posts):
    inner = rng.choice(np.arange(1, n2), posts - 2, replace=False) if posts > 2 else np.zeros(0, np.int64)
    return [0, n2] + [int(v) for v in inner]


def _feat_spec(C, bs0, bs1, ps, pl, coupled, p3=None, seed=1, short_x1=None):
    """Two floors (short blocks: ps posts, long blocks: pl posts); with p3 a third floor of p3 posts taken by the odd channels of long
    blocks (so the last channel's floor and the biggest floor differ between setups). short_x1: xs[1] of the short floor (a value
    past n makes the rendered kind's gather fail, as the reference's IndexError)."""
    from parseoggvorbis_amd.binding import SetupSpec
    rng = np.random.default_rng(seed)
    fs = _xs(rng, bs0 // 2, ps)
    if short_x1 is not None:
        fs[1] = short_x1
    floors = [(int(rng.integers(1, 5)), fs), (int(rng.integers(1, 5)), _xs(rng, bs1 // 2, pl))]
    ch1 = [1] * C
    if p3:
        floors.append((int(rng.integers(1, 5)), _xs(rng, bs1 // 2, p3)))
        ch1 = [1 if c % 2 == 0 else 2 for c in range(C)]
    coup = [(c, c + 1) for c in range(0, C - 1, 2)] if coupled else []
    return SetupSpec(C, bs0, bs1, floors, [(coup, [0] * C), (coup, ch1)], [(0, 0), (1, 1)])


CONFIGS = [  # C, bs0, bs1, short posts, long posts, coupled, third floor posts
    (1, 64, 64, 2, 9, False, None),
    (2, 256, 2048, 9, 65, True, None),
    (2, 128, 1024, 2, 29, True, 17),
    (6, 512, 4096, 9, 40, False, 65),
    (6, 4096, 8192, 65, 30, True, None),
    (2, 8192, 8192, 17, 65, False, None),
]


def _options(spec):
    big = max(len(x) for _, x in spec.floors)
    n0 = spec.blocksize0
    fl = []
    for d in sorted({max(1, big - 5), big, big + 7, 1}):
        fl += [("floor_final_ys", d, {}), ("floor_final_ys", d, {"only_biggest_floor": True}),
               ("floor_final_ys_rendered", d, {}), ("floor_final_ys_rendered", d, {"sorted_xs": True, "floor_always_positive": True}),
               ("floor_final_ys_rendered", d, {"xs_from_biggest_floor": True}),
               ("floor_final_ys_rendered", d, {"upscale_xs_factor": 2, "xs_from_biggest_floor": True, "include_floor_number": False})]
    res = []
    for kind in ("residue_ys", "residue_ys_with_floor"):
        res += [(kind, big, {}), (kind, big + 7, {"sorted_xs": True, "log1p_abs_space": True, "floor_base_factor": 2}
                                  if kind.endswith("floor") else {"sorted_xs": True, "log1p_abs_space": True}),
                (kind, big, {"scale": 0.5, "clip_abs_max": 0.3}), (kind, 1, {"ignore_xs": True}),
                (kind, n0 // 2, {"ignore_xs": True, "scale": 2.0}), (kind, max(1, big - 1), {})]
    return fl + res


def _check_against_model(feats, spec, b, seed_what):
    from parseoggvorbis_amd.binding import Synth, VsynError
    from tests import feature_model as fm
    taps = fm._taps(spec, b)
    s = Synth(spec, device=0, max_streams=len(b["segments"]))
    for kind, dim, kw in _options(spec):
        what = (seed_what, kind, dim, kw)
        try:
            want = fm.model_features(spec, b, kind, dim, taps=taps, **kw)
            werr = None
        except fm.ModelError as e:
            want, werr = None, e
        fs = feats.feature_spec(dim, kind, **kw)
        if werr is not None and werr.reason == "assert":
            with pytest.raises(VsynError):
                s.features_host(fs, b["packets"], b["segments"], b["ys"], b["residue"])
            continue
        got = s.features_host(fs, b["packets"], b["segments"], b["ys"], b["residue"])
        if werr is not None:
            assert got["rc"] != 0 and got["flags"] & (1 << 8), (what, werr, got["flags"])
            continue
        assert got["rc"] == 0, (what, got["flags"])
        assert [m.shape[0] for m in want] == list(got["seg_rows"]), what
        off = np.concatenate([[0], np.cumsum(got["seg_rows"])]).astype(int)
        for g, m in enumerate(want):
            assert_close(got["rows"][off[g]:off[g + 1]], m, kind, what + (g,), kw)


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "C%d_%d_%d_p%d_%d%s_f3%s" % (c[0], c[1], c[2], c[3], c[4], "c" if c[5] else "", c[6]))
def test_random_batches_equal_the_model(feats, cfg):
    """Block-size pairs 64/64 .. 8192/8192; 1, 2 and 6 channels with and without coupling; floors of 2 to 65 posts, two or three
    floors (the biggest-floor rule, xs_from_biggest_floor, the floor_base carry over packets without a biggest-floor channel);
    unused_frac 0.3; output_dim below, equal to and above the post count, 1, and ignore_xs up to n/2; three segments."""
    from tests.workloads import synth_batch
    C, bs0, bs1, ps, pl, coupled, p3 = cfg
    spec = _feat_spec(C, bs0, bs1, ps, pl, coupled, p3, seed=bs1 + C)
    b = synth_batch(spec, 3, 14, "mixed", seed=bs0 + pl, unused_frac=0.3, ylo=20, yhi=70)
    _check_against_model(feats, spec, b, cfg)


def test_xs_past_the_floor_vector_fails_like_the_reference(feats):
    """A short-block floor whose xs reach n (the reference's floor vector has n entries): the rendered kind's gather raises IndexError
    there, so the device flags VSYN_ST_FEATURE_INDEX and the model says "index"; clipped by xs_from_biggest_floor it is fine."""
    from parseoggvorbis_amd.binding import Synth
    from tests import feature_model as fm
    from tests.workloads import synth_batch
    spec = _feat_spec(2, 256, 2048, 9, 29, True, seed=3, short_x1=256)
    b = synth_batch(spec, 2, 12, "mixed", seed=8)
    with pytest.raises(fm.ModelError) as ei:
        fm.model_features(spec, b, "floor_final_ys_rendered", 20)
    assert ei.value.reason == "index"
    s = Synth(spec, device=0, max_streams=2)
    got = s.features_host(feats.feature_spec(20, "floor_final_ys_rendered"), b["packets"], b["segments"], b["ys"], b["residue"])
    assert got["rc"] != 0 and got["flags"] & (1 << 8)
    _check_against_model(feats, spec, b, "short_x1=n")  # the other kinds / options on the same batch


def test_device_entry_points(feats):
    """vsyn_feature_rows_device sizes the output, vsyn_features_device fills it on the caller's stream: equal to vsyn_features_host.
    A max_seg_packets below a segment's length flags VSYN_ST_BAD_SEGMENT; no packets at all still writes the (zero) offsets."""
    import ctypes as C
    import torch
    from parseoggvorbis_amd.binding import Status, Synth
    from tests.workloads import fixture_like_spec, synth_batch
    spec = fixture_like_spec(2)
    b = synth_batch(spec, 4, 20, "mixed", seed=21, unused_frac=0.3)
    s = Synth(spec, device=0, max_streams=4)
    dev = torch.device("cuda:0")
    P, S = len(b["packets"]), len(b["segments"])
    d_pk = torch.from_numpy(b["packets"].view(np.uint8).copy()).to(dev)
    d_seg = torch.from_numpy(b["segments"].view(np.uint8).copy()).to(dev)
    d_ys = torch.from_numpy(b["ys"].view(np.int16).copy()).to(dev)
    d_res = torch.from_numpy(b["residue"]).to(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    err, st = C.c_char_p(), Status()
    for kind, dim, kw in (("floor_final_ys_rendered", 33, {}), ("residue_ys_with_floor", 40, {"log1p_abs_space": True})):
        fs = feats.feature_spec(dim, kind, **kw)
        want = s.features_host(fs, b["packets"], b["segments"], b["ys"], b["residue"])
        d_off = torch.full((S + 1,), -1, dtype=torch.int64, device=dev)
        assert s.lib.vsyn_feature_rows_device(s.h, C.byref(fs), P, d_pk.data_ptr(), S, d_seg.data_ptr(), 20, d_off.data_ptr(), stream,
                                              C.byref(err)) == 0, err.value
        torch.cuda.synchronize()
        off = d_off.cpu().numpy()
        assert np.array_equal(np.diff(off), want["seg_rows"].astype(np.int64)) and off[0] == 0
        d_rows = torch.full((int(off[-1]), dim), float("nan"), dtype=torch.float32, device=dev)
        d_off2 = torch.zeros(S + 1, dtype=torch.int64, device=dev)
        assert s.lib.vsyn_features_device(s.h, C.byref(fs), P, d_pk.data_ptr(), S, d_seg.data_ptr(), 20, d_ys.data_ptr(), d_res.data_ptr(),
                                          d_rows.data_ptr(), d_off2.data_ptr(), stream, C.byref(err)) == 0, err.value
        assert s.lib.vsyn_sync_status(s.h, stream, C.byref(st), C.byref(err)) == 0, st.flags
        assert np.array_equal(d_off2.cpu().numpy(), off)
        assert np.array_equal(d_rows.cpu().numpy().view(np.uint32), want["rows"].view(np.uint32))
        # max_seg_packets below the segments' 20 packets: flagged, nothing written past the grid
        assert s.lib.vsyn_features_device(s.h, C.byref(fs), P, d_pk.data_ptr(), S, d_seg.data_ptr(), 10, d_ys.data_ptr(), d_res.data_ptr(),
                                          d_rows.data_ptr(), d_off2.data_ptr(), stream, C.byref(err)) == 0, err.value
        assert s.lib.vsyn_sync_status(s.h, stream, C.byref(st), C.byref(err)) != 0 and st.flags & (1 << 5)
    # no packets, two empty segments: the offsets are still written
    empty = b["segments"][:2].copy()
    empty["num_packets"], empty["first_packet"], empty["residue_off"] = 0, 0, 0
    d_e = torch.from_numpy(empty.view(np.uint8).copy()).to(dev)
    d_off = torch.full((3,), -1, dtype=torch.int64, device=dev)
    assert s.lib.vsyn_feature_rows_device(s.h, C.byref(fs), 0, None, 2, d_e.data_ptr(), 0, d_off.data_ptr(), stream, C.byref(err)) == 0
    assert s.lib.vsyn_sync_status(s.h, stream, C.byref(st), C.byref(err)) == 0
    assert d_off.cpu().numpy().tolist() == [0, 0, 0]
