#!/usr/bin/env python3
"""Generate tests/golden/ref_shim.npz: the answers of the REFERENCE's own code (oracle/_ref/libref_shim.so, built by
oracle/Makefile from the reference's sources) on the seeded inputs of tests/test_oracle_vs_ref.py, so that the test pins
the oracle against the reference without the reference tree.  TEST INFRASTRUCTURE, run where the reference is present:

    make -C oracle && python oracle/make_ref_vectors.py

Arrays up to INLINE_BYTES are stored as they are; larger ones as the sha256 of their bits (tests/test_oracle_vs_ref.digest).
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import oracle_binding as ob  # noqa: E402
from tests import test_oracle_vs_ref as t  # noqa: E402

INLINE_BYTES = 16384


def main():
    assert ob.have_ref(), "%s not built (make -C oracle where the reference sources are present)" % ob.REF_SHIM
    ref = ob.ref()
    out = {}

    def put(key, a):
        a = np.ascontiguousarray(a)
        out[key] = a if a.nbytes <= INLINE_BYTES else np.array(t.digest(a))

    for n in t.SIZES:
        trig = np.zeros(n + n // 4, np.float32)
        rev = np.zeros(n // 4, np.int32)
        ref.ref_mdct_tables(n, ob.p(trig), ob.p(rev))
        put("mdct_trig_%d" % n, t.bits(trig))
        put("mdct_bitrev_%d" % n, rev)
        x = t.mdct_input(n)
        want = np.empty((x.shape[0], n), np.float32)
        ref.ref_mdct_backward_batch(n, x.shape[0], ob.p(x), ob.p(want))
        put("mdct_backward_%d" % n, t.bits(want))

    for n in t.CLOSED_FORM_SIZES:
        x = t.closed_form_input(n)
        want = np.empty(n, np.float32)
        ref.ref_mdct_backward(n, ob.p(x), ob.p(want))
        out["closed_form_%d" % n] = want  # the test needs the values (tolerance, symmetries)

    for bs0, bs1 in t.WINDOW_PAIRS:
        for flag, prev, nxt in t.WINDOW_CASES:
            a = np.zeros(bs1 if flag else bs0, np.float32)
            assert ref.ref_window(bs0, bs1, flag, prev, nxt, ob.p(a)) == 0
            put("window_%d_%d_%d%d%d" % (bs0, bs1, flag, prev, nxt), t.bits(a))

    put("inverse_db_table", t.bits(np.ctypeslib.as_array(ref.ref_inverse_db_table(), shape=(256,))))

    points, lines, sets = t.render_inputs()
    put("render_point", np.array([ref.ref_render_point(*(int(v) for v in pt)) for pt in points], np.uint32))
    rendered = []
    for x0, y0, x1, y1, ln in lines:
        b = np.full(ln, 7777, np.uint32)
        ref.ref_render_line(x0, y0, x1, y1, ob.p(b), ln)
        rendered.append(b)
    put("render_line", np.concatenate(rendered))
    put("neighbors", np.array([(ref.ref_low_neighbor(ob.p(v), len(v), idx), ref.ref_high_neighbor(ob.p(v), len(v), idx))
                               for v in sets for idx in range(1, len(v))], np.int32))

    def floor1(key, cases, accepted=False):
        failed, decoded = [], []
        for xs, mult, ys, n in cases:
            want = np.zeros(n, np.float32)
            rr = ref.ref_floor1_synth(ob.p(xs), len(xs), mult, ob.p(ys), n, ob.p(want))
            assert not (accepted and rr), "%s: the reference rejects a case of the table (fix its generator)" % key
            failed.append(rr != 0)
            if rr == 0:
                decoded.append(t.bits(want))
        out[key + "_failed"] = np.array(failed, bool)
        put(key, np.concatenate(decoded) if decoded else np.zeros(0, np.uint32))

    for mult in t.FLOOR_MULTS:
        for posts, n in t.FLOOR_SHAPES:
            floor1("floor1_%d_%d_%d" % (mult, posts, n), [(xs, mult, ys, n) for xs, ys in t.floor1_inputs(mult, posts, n)])
    for geom in t.fg.GEOMETRIES:  # x[1] above / below half the block size, floors shared by both block sizes
        for bs0, bs1 in t.fg.PAIRS:
            floor1(*t.geometry_floor1_inputs(geom, bs0, bs1), accepted=True)

    for bs0, bs1, channels in t.OVERLAP_CONFIGS:
        for trial, c in enumerate(t.overlap_inputs(bs0, bs1, channels)):
            npk, cap = len(c["flags"]), c["cap"]
            want = np.zeros((channels, cap), np.float32)
            emit = np.zeros(npk, np.uint32)
            bad = C.c_int(-1)
            flat = np.concatenate([b.ravel() for b in c["blocks"]])
            rc = ref.ref_overlap_add(channels, bs0, bs1, npk, ob.p(c["flags"]), ob.p(c["widx"]), ob.p(c["gran"]), ob.p(flat),
                                     ob.p(want), cap, ob.p(emit), C.byref(bad))
            assert rc == 0 and np.isfinite(want).all()
            key = "overlap_%d_%d_%d_%d" % (bs0, bs1, channels, trial)
            put(key + "_emit", emit)
            put(key + "_pcm", t.bits(t.canonical_zero(want)))

    for bs0, bs1, channels in t.WINFLAG_CONFIGS:
        for trial, c in enumerate(t.winflag_inputs(bs0, bs1, channels)):
            rc, emit, want = t.overlap_ref_call(ref, "ref_overlap_add", bs0, bs1, channels, c)
            assert rc == 0 and np.isfinite(want).all()
            key = "winflags_%d_%d_%d_%d" % (bs0, bs1, channels, trial)
            put(key + "_emit", emit)
            put(key + "_pcm", t.bits(t.canonical_zero(want)))

    np.savez_compressed(t.REF_VECTORS, **out)
    print("wrote %s: %d entries, %d bytes" % (t.REF_VECTORS, len(out), os.path.getsize(t.REF_VECTORS)))


if __name__ == "__main__":
    main()
