"""Feature matrices (parseoggvorbis_amd/features.py): what needs no GPU — argument checks before the library loads, the
committed reference goldens' shape, and the new C-ABI symbols."""
import json
import os

import numpy as np
import pytest

from parseoggvorbis_amd import features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = ["test.stereo44khz", "test.mono44khz"] + ["synth_%02d" % i for i in range(16)] + ["winflags_bcd"]


def test_concat_residue_is_refused_by_name():
    with pytest.raises(features.FeatureError) as ei:
        features.get_features_from_raw_bytes(b"", 10, kind="floor_final_ys_rendered_concat_residue")
    assert "floor_final_ys_rendered_concat_residue" in str(ei.value)
    assert "residue_ys_with_floor" in str(ei.value)  # names what is supported


def test_bad_kind_is_refused_with_the_kind_names():
    with pytest.raises(features.FeatureError) as ei:
        features.get_features_from_raw_bytes(b"", 10, kind="mfcc")
    msg = str(ei.value)
    assert "'mfcc'" in msg
    for k in ("floor_final_ys", "floor_final_ys_rendered", "residue_ys", "residue_ys_with_floor"):
        assert k in msg


@pytest.mark.parametrize("kind,kw", [("floor_final_ys", {"scale": 2.0}), ("residue_ys", {"upscale_xs_factor": 2}),
                                     ("residue_ys_with_floor", {"only_biggest_floor": True}), ("floor_final_ys_rendered", {"bogus": 1})])
def test_kwargs_of_the_other_reader_are_refused(kind, kw):
    with pytest.raises(TypeError) as ei:
        features.get_features_from_raw_bytes(b"", 10, kind=kind, **kw)
    assert kind in str(ei.value) and list(kw)[0] in str(ei.value)


def test_reference_asserts_are_kept():
    with pytest.raises(AssertionError):
        features.feature_spec(10, "floor_final_ys", only_biggest_floor=True, include_floor_number=True)
    with pytest.raises(features.FeatureError):
        features.feature_spec(0, "residue_ys")


def test_spec_encoding():
    s = features.feature_spec(12, "floor_final_ys_rendered", sorted_xs=True, upscale_xs_factor=2, xs_from_biggest_floor=True)
    assert (s.kind, s.output_dim, s.upscale_xs_factor) == (2, 12, 2.0)
    assert s.options == features.OPT_INCLUDE_FLOOR_NUMBER | features.OPT_SORTED_XS | features.OPT_XS_FROM_BIGGEST_FLOOR
    s = features.feature_spec(12, "floor_final_ys", only_biggest_floor=True)
    assert s.options == features.OPT_ONLY_BIGGEST_FLOOR  # the floor-number column goes with it, as in the reference
    s = features.feature_spec(70, "residue_ys_with_floor", clip_abs_max=0.0, scale=0.5, log1p_abs_space=True, floor_base_factor=2)
    assert s.options == features.OPT_LOG1P_ABS_SPACE and s.scale == 0.5 and s.floor_base_factor == 2.0  # clip 0 = off
    s = features.feature_spec(70, "residue_ys", clip_abs_max=0.8, ignore_xs=True)
    assert s.options == features.OPT_CLIP | features.OPT_IGNORE_XS and abs(s.clip_abs_max - 0.8) < 1e-7


def test_shim_has_the_reference_interface():
    lib = features.ParseOggVorbisLib.get_instance()
    assert lib is features.ParseOggVorbisLib.get_instance()
    with pytest.raises(features.FeatureError):
        lib.get_features_from_raw_bytes(b"", 10, kind="nope")


@pytest.mark.parametrize("name", FILES)
def test_goldens_are_complete(name):
    z = np.load(os.path.join(GOLDEN, "features_%s.npz" % name))
    grid = json.loads(str(z["grid"]))
    assert len(grid) >= 16
    for i, (kind, dim, kw) in enumerate(grid):
        assert ("c%d" % i in z.files) != ("e%d" % i in z.files)
        if "c%d" % i in z.files:
            m = z["c%d" % i]
            assert m.dtype == np.float32 and m.ndim == 2 and m.shape[1] == dim and m.shape[0] > 0
            assert np.isfinite(m).all()


def test_new_symbols_are_exported():
    from parseoggvorbis_amd import binding
    lib = binding.load()
    for s in ("vsyn_feature_rows_device", "vsyn_features_device", "vsyn_features_host"):
        assert s in binding.declared_symbols() and hasattr(lib, s)
    import ctypes
    host = ctypes.CDLL(features.HOST_LIB_PATH)
    assert hasattr(host, "ogg_vorbis_features_corpus")
    assert ctypes.sizeof(binding.FeatureSpec) == 40


# ---- the independent model (tests/feature_model.py) against the reference's own matrices ----

import subprocess  # noqa: E402

import __graft_entry__ as entry  # noqa: E402
from tests import feature_model as fm  # noqa: E402
from tests.workloads import load_golden, read_entropy_dump  # noqa: E402

HOST = os.path.join(ROOT, "parseoggvorbis_amd", "host")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    entry.build_hip()
    entry.build_host()
    out = str(tmp_path_factory.mktemp("probe") / "host_entropy_dump")
    csrc = os.path.join(ROOT, "parseoggvorbis_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O2", "-o", out, os.path.join(ROOT, "tests", "host_entropy_dump.cpp"),
                    "-L" + HOST, "-lparseoggvorbis_amd", "-L" + csrc, "-lvorbis_synth_hip", "-Wl,-rpath," + HOST,
                    "-Wl,-rpath," + csrc, "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    return out


def fixture_batch(name, probe, tmp_path):
    """(spec, batch) of a committed fixture: the real files from their golden dump, the synthetic ones from the host's entropy half
    (float residue) and the setup recorded next to them."""
    if name.startswith("test."):
        spec, b, _ = load_golden(name)
        return spec, b
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    out = str(tmp_path / "e.bin")
    r = subprocess.run([probe, os.path.join(GOLDEN, name + ".ogg"), out], capture_output=True, text=True,
                       env=dict(os.environ, PARSEOGGVORBIS_VQ="0"))
    assert r.returncode == 0, r.stderr
    d = read_entropy_dump(out)
    spec = fm.spec_from_synth_npz(z)
    assert d["ys_stride"] == spec.ys_stride
    from parseoggvorbis_amd.binding import SEGMENT_DTYPE
    seg = np.zeros(1, SEGMENT_DTYPE)
    seg["num_packets"], seg["flags"] = d["P"], 1
    return spec, dict(packets=d["packets"], segments=seg, ys=d["ys"], residue=d["residue"])


def ulp_close(got, want, k):
    return np.abs(got.astype(np.float64) - want) <= k * np.spacing(np.maximum(np.abs(got), np.abs(want)))


@pytest.mark.parametrize("name", FILES)
def test_model_reproduces_every_golden_matrix(name, probe, tmp_path):
    spec, b = fixture_batch(name, probe, tmp_path)
    taps = fm._taps(spec, b)
    z = np.load(os.path.join(GOLDEN, "features_%s.npz" % name))
    for i, (kind, dim, kw) in enumerate(json.loads(str(z["grid"]))):
        what = (name, i, kind, dim, kw)
        if "e%d" % i in z.files:
            with pytest.raises(fm.ModelError) as ei:
                fm.model_features(spec, b, kind, dim, taps=taps, **kw)
            assert ei.value.reason == "broadcast" and "broadcast" in str(z["e%d" % i]), what
            continue
        got = fm.model_features(spec, b, kind, dim, taps=taps, **kw)[0]
        want = z["c%d" % i]
        assert got.shape == want.shape, what
        if kind.startswith("floor"):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what
        else:
            assert ulp_close(got, want, 2).all(), what


def test_model_zoom_matches_scipy():
    scipy_ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1)
    n = 0
    for it in range(600):
        L = int(rng.integers(2, 66))
        z = [2, 3, 4, 0.5, 1.5, 2.5, 8, 0.25][it % 8]
        xs = rng.integers(0, 4097, L)
        xs[0], xs[1] = 0, 1024
        if it % 3 == 0:
            xs = np.sort(xs)
        got = fm.zoom_round([int(v) for v in xs], z)
        if got is None:
            assert round(L * z) != L * z
            continue
        want = np.round(scipy_ndimage.zoom(np.array(xs, dtype="float32"), zoom=z, order=1, mode="nearest")).astype("int32")
        assert np.array_equal(np.array(got), want), (L, z)
        n += 1
    assert n > 300
