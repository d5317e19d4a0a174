"""Floor-1 X lists whose x[1] is not half the block size (floor_geometry_cases.py), on the CPU: the oracle against the plain
integer model of the case table, through OracleSynth.submit_host — the only place where a floor that both modes share meets two
block sizes. (The oracle's floor tail against the REFERENCE on the same rows: test_oracle_vs_ref.py, golden/ref_shim.npz.)
Every geometry x block-size pair runs; nothing is filtered."""
import numpy as np
import pytest

from oracle import oracle_binding as ob
from tests import floor_geometry_cases as fg
from tests import synth_model as sm

CHANNELS = {(256, 2048): (2, 1)}  # stereo coupled everywhere, mono too on 256/2048


def batches(geom, bs0, bs1):
    """-> [(spec, kind, batch)]: the mixed and the all-long batch of every channel count of the pair (the GPU module runs the same)"""
    out = []
    for channels in CHANNELS.get((bs0, bs1), (2,)):
        spec = fg.make_spec(geom, bs0, bs1, channels)
        out += [(spec, kind, fg.make_batch(spec, kind)) for kind in ("mixed", "long")]
    return out


def test_case_table_is_whole():
    """Every geometry gives, for every pair, floors with the x[1] its name promises, and every directed row of every multiplier
    lands on a short and on a long packet of the mixed batch."""
    for geom in fg.GEOMETRIES:
        for bs0, bs1 in fg.PAIRS:
            h0, h1 = bs0 // 2, bs1 // 2
            lists = fg.floor_lists(geom, bs0, bs1)
            assert len(lists) == (1 if geom in fg.SHARED else 2)
            for xs, h in zip(lists, (h0, h1)):
                assert xs[0] == 0 and xs[1] == max(xs) and len(set(xs)) == len(xs) <= 65
                assert xs[1] & (xs[1] - 1) == 0 and xs[1] <= 32768  # 1 << rangebits, rangebits a 4-bit field
                want = dict(beyond2=2 * h, beyond_max_a=32768, beyond_max_b=32768, short_of_half=h // 2, short_of_quarter=h // 4,
                            short_of_one=1, shared_long=h1, shared_short=h0, steep=h)[geom]
                assert xs[1] == want, (geom, bs0, bs1, xs[1])
            if geom == "beyond2":
                for xs, h in zip(lists, (h0, h1)):
                    assert 12 <= len(xs) <= 20 and {h - 1, h, h + 1} <= set(xs) and sum(x > h + 1 for x in xs[2:]) >= 3
            if geom == "beyond_max_b":
                for xs, h in zip(lists, (h0, h1)):
                    s = sorted(xs)
                    inside = [x for x in s if x < h]
                    assert len(xs) == 20 and s[len(inside)] - inside[-1] > 16384
            for spec, kind, b in batches(geom, bs0, bs1):
                if kind == "mixed":
                    for lng in (0, 1):
                        for m in fg.MULTS:
                            assert b["placed"][(lng, m)] == set(fg.DIRECTED), (geom, bs0, bs1, spec.channels, lng, m)


@pytest.mark.parametrize("bs0,bs1", fg.PAIRS)
@pytest.mark.parametrize("geom", fg.GEOMETRIES)
def test_oracle_taps_equal_the_integer_model(geom, bs0, bs1):
    """floor_final and floor_curve of the oracle == the integer model, bit for bit; rc 0 and no status flag; the oracle's emit
    lengths and PCM inside the per-packet gate of synth_model.py."""
    for spec, kind, b in batches(geom, bs0, bs1):
        ctx = (geom, bs0, bs1, spec.channels, kind)
        w = ob.OracleSynth(spec, len(b["segments"])).submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"],
                                                                 want_taps=True)
        assert (w["rc"], w["flags"], w["first_bad"]) == (0, 0, 0xFFFFFFFF), ctx
        final, crv = fg.model_taps(spec, b)
        assert np.array_equal(w["taps"]["floor_final"], final), ctx
        assert np.array_equal(w["taps"]["floor_curve"], crv), ctx
        sm.check_model(w, spec, b, ctx=ctx)  # (asserts the model's frame counts too)
