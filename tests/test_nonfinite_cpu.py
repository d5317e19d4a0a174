"""The rule for Inf and NaN values (include/vorbis_synth_hip.h: step 8 of "spectral features", step 6 of "linear spectra", step 3 of
"resampling", step 5 of "spectral post-processing", rule 7 of "PCEN", the VSYN_PCM_S16 line) settled on the float64 models before
tests/test_gpu_nonfinite.py holds the device to it: fed the dirty batches of tests/nonfinite_cases.py, a model's values that are not
finite are exactly the helper's footprint, and everywhere else the model equals its own clean output. Also the conditions the GPU
tests rely on (no empty mel band, segments no shorter than the delta window, the tile of every shape) and the helper's own
arithmetic (the float32 fma, the int16 restatement).

The mel model builds an n_fft x (n_fft / 2 + 1) matrix, so it runs at the 64-point shape only; the 8192-point shapes of the GPU
module differ in the tile, which is no part of the rule, and are checked here for their tile and their bands."""
from fractions import Fraction

import numpy as np
import pytest

from tests import nonfinite_cases as nf
from tests import pcen_model as pm
from tests import resample_model as rm
from tests import spectral_lin_model as lm
from tests import spectral_model as sm
from tests import spectral_post_model as spm


def _lin(x, kind, n, hop, win, center, power=2, top_db=None):
    with np.errstate(all="ignore"):
        X, _ = lm.stft(x, n, hop, win, center)
        if kind == "stft":
            return X
        S = X.real * X.real + X.imag * X.imag
        S = np.sqrt(S) if power == 1 else S
        return S if kind == "lin_power" else sm.clamp_top_db(10.0 * np.log10(np.maximum(S, 1e-10)), top_db)


def _mel(x, kind, n, hop, win, center, **kw):
    with np.errstate(all="ignore"):
        return sm.spectral(x, nf.MEL_SR, kind=kind, n_fft=n, hop_length=hop, win_length=win, center=center, n_mels=nf.N_MELS, **kw)[0]


def _check_rows(clean, dirty, hit, what):
    """Rows of `hit`: no finite value; other rows: the clean model's, exactly (NaN never occurs there)."""
    assert clean.shape == dirty.shape and hit.shape == (clean.shape[0],), what
    assert np.isfinite(clean).all(), what
    assert np.array_equal(dirty[~hit], clean[~hit]), what
    assert not np.isfinite(dirty[hit]).any(), (what, np.argwhere(np.isfinite(dirty[hit]))[:4])


def _spectral_cases(shape, model, kinds):
    n, hop, win, center, lengths, tile = shape
    T = lengths[nf.DIRTY_SEG]
    pcm, _ = nf.pcm_batch(lengths, 2, seed=n + hop)
    pos = nf.spectral_positions(T, n, hop, win, center, tile)
    for kind, kw in kinds:
        clean = model(pcm[nf.DIRTY_SEG, :, :T], kind, n, hop, win, center, **kw)
        for name, vname in nf.cases(pos):
            x = nf.dirtied(pcm, nf.writes_of(name, pos[name], vname))[nf.DIRTY_SEG, :, :T]
            hit = nf.spectral_footprint(pos[name], T, n, hop, win, center)
            if name == "behind":
                assert not hit.any()
            elif name != "first" or center or win == n:
                assert hit.any() and not hit.all()
            _check_rows(clean, model(x, kind, n, hop, win, center, **kw), hit, (shape[:4], kind, kw, name, vname))


@pytest.mark.parametrize("shape", nf.LIN_SHAPES, ids=lambda s: "n%d_h%d_w%d_%s" % (s[0], s[1], s[2], "c" if s[3] else "nc"))
def test_linear_models_footprint(shape):
    assert nf.lin_tile(shape[0], shape[1]) == shape[5]
    _spectral_cases(shape, _lin, nf.LIN_KINDS)


def test_a_sample_inside_the_frame_but_outside_the_window_support_touches_nothing():
    n, hop, win, center, lengths, _ = nf.LIN_SHAPES[1]
    assert win < n and not center and not nf.spectral_footprint([0], lengths[1], n, hop, win, center).any()


@pytest.mark.parametrize("shape", [s for s in nf.MEL_SHAPES if s[0] == 64], ids=lambda s: "n%d_h%d_w%d_%s" % (s[0], s[1], s[2], "c" if s[3] else "nc"))
def test_mel_model_footprint(shape):
    _spectral_cases(shape, _mel, nf.MEL_KINDS)


def test_mel_shapes_have_the_tiles_and_no_empty_band():
    """An empty band would give a finite 0 inside a dirty frame on the device, whose bands are sparse."""
    assert [nf.mel_tile(s[0], s[1], nf.N_MELS) for s in nf.MEL_SHAPES] == [s[5] for s in nf.MEL_SHAPES] == [16, 16, 16, 4, 1]
    assert sum(not s[3] for s in nf.MEL_SHAPES) == 2 and any(not s[3] and s[2] < s[0] for s in nf.MEL_SHAPES)
    for n in sorted({s[0] for s in nf.MEL_SHAPES} | {s[1] for s in nf.TOP_DB_SHAPES if s[0] != "lin_db"}):
        W = sm.mel_filters(nf.MEL_SR, n, nf.N_MELS).astype(np.float32)
        assert (W.max(axis=1) > 0).all(), n
    for n, hop, win, center, lengths, tile in nf.MEL_SHAPES + nf.LIN_SHAPES:
        F = [sm.num_frames(T, n, hop, center) for T in lengths]
        assert F[1] > tile and min(F) >= 1 and len(set(lengths)) == 3


@pytest.mark.parametrize("kind,n,hop,extra,center", nf.TOP_DB_SHAPES, ids=nf.TOP_DB_IDS)
def test_top_db_takes_the_maximum_over_finite_values_and_leaves_the_others(kind, n, hop, extra, center):
    """The model with top_db against the rule stated on its own top_db = 0 rows: outside the footprint max(D0, max of D0 outside the
    footprint - top_db), exactly; with the clean maximum inside the footprint (a sample in the loud stretch) and outside it."""
    T = nf.TOP_DB_LENGTHS[nf.DIRTY_SEG]
    pcm, _ = nf.pcm_batch(nf.TOP_DB_LENGTHS, 2, seed=5, burst=nf.TOP_DB_BURST)
    model = _lin if kind == "lin_db" else _mel
    db_kind = "lin_db" if kind == "lin_db" else "mel_db"
    kw = {k: v for k, v in extra.items() if k != "n_mels"}
    D0 = model(pcm[1, :, :T], db_kind, n, hop, n, center, top_db=None)
    row_max = int(np.argmax(D0.max(axis=1)))
    for where, s in (("inside", nf.TOP_DB_BURST[0] + nf.TOP_DB_BURST[1] // 2), ("outside", 0)):
        hit = nf.spectral_footprint([s], T, n, hop, n, center)
        assert hit[row_max] == (where == "inside")
        for top_db in nf.TOP_DB:
            for vname in nf.VALUES:
                x = nf.dirtied(pcm, [(s, nf.VALUES[vname])])[1, :, :T]
                got = model(x, kind, n, hop, n, center, top_db=top_db, **kw)
                want = np.maximum(D0, D0[~hit].max() - top_db) if top_db else D0
                if top_db:
                    assert (want[~hit] > D0[~hit]).any()  # the clamp is at work in the rows that are compared
                if kind == "mfcc":  # the matrix product rounds in float64: |D| < 200 dB over 8 terms, far below 1e-9
                    want = want @ sm.dct_ortho(nf.N_MFCC, nf.N_MELS).T
                    assert np.allclose(got[~hit], want[~hit], rtol=0, atol=1e-9)
                else:
                    assert np.array_equal(got[~hit], want[~hit]), (where, top_db, vname)
                assert not np.isfinite(got[hit]).any() and np.isfinite(got[~hit]).all()


@pytest.mark.parametrize("r_in,r_out,lengths", nf.RS_SHAPES, ids=["%d_%d" % s[:2] for s in nf.RS_SHAPES])
def test_resample_model_footprint(r_in, r_out, lengths):
    T = lengths[nf.DIRTY_SEG]
    pcm, _ = nf.pcm_batch(lengths, 2, seed=r_in % 1000)
    up, down = rm.ratio(r_in, r_out)
    K = -(-(20 * max(up, down) + 1) // up)
    assert rm.padded_taps(20 * max(up, down) + 1, up) > K  # every pair here has padded taps: the footprint by K4 is wider than by K
    pos = nf.resample_positions(T, r_in, r_out)
    assert "tile" in pos
    with np.errstate(all="ignore"):
        clean = rm.resample(pcm[1, :, :T], r_in, r_out)
        for name, vname in nf.cases(pos):
            dirty = rm.resample(nf.dirtied(pcm, nf.writes_of(name, pos[name], vname))[1, :, :T], r_in, r_out)
            hit = nf.resample_footprint(pos[name], T, r_in, r_out)
            assert hit.any() and not hit.all()
            assert np.array_equal(dirty[1 - nf.DIRTY_CH], clean[1 - nf.DIRTY_CH])
            _check_rows(clean[nf.DIRTY_CH][:, None], dirty[nf.DIRTY_CH][:, None], hit, (r_in, r_out, name, vname))


def test_pcen_model_footprint():
    """A NaN and a -Inf poison their column from their row on. A +Inf does not (rule 7): its row is NaN, and the rows behind it are
    the 0 that a gain of 0 gives, for every form of the compression."""
    F, D, d = nf.PCEN_ROWS[1], nf.PCEN_D, nf.PCEN_COL
    rows, first = nf.rows_batch(nf.PCEN_ROWS, D, seed=3, positive=True)
    x = rows[first[1]:first[2]]
    for extra in (dict(), dict(bias=0.0), dict(power=0.0)):
        clean = pm.pcen(x, **nf.PCEN_KW, **extra)
        assert np.isfinite(clean).all()
        for f in nf.PCEN_DIRTY_ROWS:
            for vname, v in nf.VALUES.items():
                bad = x.copy()
                bad[f, d] = v
                got = pm.pcen(bad, **nf.PCEN_KW, **extra)
                if vname == "+inf":
                    hit, forced = nf.pcen_plus_inf(f, d, F, D)
                    assert (got[forced] == 0).all(), (extra, f)
                    same = ~(hit | forced)
                else:
                    hit = nf.pcen_footprint(f, d, F, D)
                    same = ~hit
                assert not np.isfinite(got[hit]).any() and np.array_equal(nf.bits(got)[same], nf.bits(clean)[same]), (extra, f, vname)
    # with gain = 0 the gain of a column whose M is +Inf is exp(-0 * Inf) = NaN: the column is NaN from the row on
    bad = x.copy()
    bad[70, d] = np.inf
    assert np.array_equal(np.isfinite(pm.pcen(bad, gain=0.0, **nf.PCEN_KW)), ~nf.pcen_footprint(70, d, F, D))


@pytest.mark.parametrize("order", nf.POST_ORDERS)
@pytest.mark.parametrize("width", nf.POST_WIDTHS)
def test_post_model_footprint(order, width):
    assert min(nf.POST_ROWS) >= max(nf.POST_WIDTHS)  # every segment has at least `width` rows
    F, D, d = nf.POST_ROWS[1], nf.POST_D, nf.POST_COL
    rows, first = nf.rows_batch(nf.POST_ROWS, D, seed=4, positive=False)
    x = rows[first[1]:first[2]]
    h = (width - 1) // 2
    for norm in (None, "mean", "mean_var"):
        with np.errstate(all="ignore"):
            clean = spm.post(x, order, width, norm)
            for f in nf.post_dirty_rows(F, width):
                for vname, v in nf.VALUES.items():
                    bad = x.copy()
                    bad[f, d] = v
                    got = spm.post(bad, order, width, norm)
                    hit = nf.post_footprint(f, d, F, D, order, width, norm is not None)
                    if f == h and norm is None:
                        assert hit[:h, D + d].all() and hit[2 * h, D + d] and not hit[2 * h + 1, D + d]  # the edge rows repeat row h
                    assert np.array_equal(got[~hit], clean[~hit]) and np.isfinite(clean).all(), (norm, f, vname)
                    assert not np.isfinite(got[hit]).any(), (norm, f, vname, np.argwhere(hit & np.isfinite(got))[:4])


def test_footprints_of_single_samples():
    """The formulas on cases small enough to count by hand."""
    # n_fft 8, hop 2, no centring, T = 20: frames start at 0, 2, .., 12; sample 5 lies in frames 0 (0..7), 1 (2..9), 2 (4..11)
    assert np.flatnonzero(nf.spectral_footprint([5], 20, 8, 2, 8, False)).tolist() == [0, 1, 2]
    # win_length 4: woff 2, supports 2..5, 4..7, 6..9, ..: sample 5 lies in frames 0 and 1
    assert np.flatnonzero(nf.spectral_footprint([5], 20, 8, 2, 4, False)).tolist() == [0, 1]
    # centred: pad 4, frame f covers f * 2 - 4 .. f * 2 + 3: sample 0 lies in frames 1 and 2 (frame 0 covers -4..3 too) -> 0, 1, 2
    assert np.flatnonzero(nf.spectral_footprint([0], 20, 8, 2, 8, True)).tolist() == [0, 1, 2]
    # 2 -> 1: up 1, down 2, H = 20, N = 41, K = 41, K4 = 44: output j reads x[2 j + 20 - 43 .. 2 j + 20]; sample 100 -> j 40 .. 61
    assert np.flatnonzero(nf.resample_footprint([100], 400, 2, 1)).tolist() == list(range(40, 62))
    # width 5 (h = 2), F = 10: row 2 is read by D rows 0 .. 4 (0 and 1 repeat row 2's), row 9 by rows 5 .. 9 (clamped to 7)
    assert np.flatnonzero(nf.delta_rows(2, 10, 5)).tolist() == [0, 1, 2, 3, 4]
    assert np.flatnonzero(nf.delta_rows(9, 10, 5)).tolist() == [7, 8, 9]


def test_fma32_is_the_single_rounding():
    rng = np.random.default_rng(0)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-9, 3, 4000)).astype(np.float32)
    # ties of the float32 rounding that only the product's low bits break: a b = 1 + 2^-24 + 2^-46, c = 0 and the like
    a = np.concatenate([a, np.float32([1 + 2.0 ** -23, 1 + 2.0 ** -23, 3.0])])
    b = np.concatenate([b, np.float32([1 + 2.0 ** -23, 1 - 2.0 ** -23, 2.0 ** -25])])
    c = np.concatenate([c, np.float32([2.0 ** -24, 2.0 ** -24, 1.0])])
    got = nf.fma32(a, b, c)
    for x, y, z, g in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        lo, hi = np.nextafter(np.float32(g), np.float32(-np.inf)), np.nextafter(np.float32(g), np.float32(np.inf))
        err = abs(Fraction(g) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), (x, y, z, g)
        if err == abs(Fraction(float(lo)) - exact) or err == abs(Fraction(float(hi)) - exact):
            assert np.float32(g).view(np.uint32) & 1 == 0  # a true tie goes to even


def test_the_int16_restatement():
    assert np.array_equal(nf.s16(nf.S16_INPUTS), nf.S16_WANT)
    assert nf.s16(np.float32([0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, 32766.5 / 32768])).tolist() == [0, 2, 2, 0, 32766]


def test_db_interval_takes_its_thresholds_from_the_finite_values():
    """lm.db_interval (the gate of the lin_db device tests) on a segment with a dirty frame: the model's rows and both ends of the
    interval are clamped against the finite values alone, the dirty frame stays as it is, and on finite input nothing moves."""
    n, hop = 64, 16
    T = nf.TOP_DB_LENGTHS[1]
    pcm, _ = nf.pcm_batch(nf.TOP_DB_LENGTHS, 2, seed=5, burst=nf.TOP_DB_BURST)
    s = nf.TOP_DB_BURST[0] + nf.TOP_DB_BURST[1] // 2
    hit = nf.spectral_footprint([s], T, n, hop, n, True)
    with np.errstate(all="ignore"):
        Sc, dSc = lm.power_bound(*lm.stft(pcm[1, :, :T], n, hop), 2)
        Sd, dSd = lm.power_bound(*lm.stft(nf.dirtied(pcm, [(s, np.nan)])[1, :, :T], n, hop), 2)
        want0, lo0, hi0 = lm.db_interval(Sc, dSc, top_db=None)
        for top_db in (80.0, 20.0):
            want, lo, hi = lm.db_interval(Sd, dSd, top_db=top_db)
            assert np.isnan(want[hit]).all() and np.isnan(lo[hit]).all() and np.isnan(hi[hit]).all()
            assert np.array_equal(want[~hit], np.maximum(want0[~hit], want0[~hit].max() - top_db))
            tl, th = lo0[~hit].max() - top_db, hi0[~hit].max() - top_db
            assert np.array_equal(lo[~hit], np.maximum(lo0[~hit], tl - lm.U * abs(tl)))
            assert np.array_equal(hi[~hit], np.maximum(hi0[~hit], th + lm.U * abs(th)))
            assert (lo[~hit] <= want[~hit]).all() and (want[~hit] <= hi[~hit]).all() and (want[~hit] > want0[~hit]).any()
            # finite input: the segment's own maximum, as before
            wc, lc, hc = lm.db_interval(Sc, dSc, top_db=top_db)
            assert np.array_equal(wc, np.maximum(want0, want0.max() - top_db)) and np.isfinite(lc).all() and np.isfinite(hc).all()
    # a segment without a finite value is not clamped
    allnan = np.full((3, 4), np.nan)
    assert np.isnan(lm.db_interval(allnan, allnan, top_db=80.0)[0]).all()


def test_the_helper_constants_are_the_kernels():
    """The positions on a tile's edge use the kernels' tile sizes, which the helper restates: they are read here in the sources, so
    that a change of either is reported and the edge cases keep testing an edge. (The footprints use no kernel constant.)"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parseoggvorbis_amd", "csrc")
    rs = open(os.path.join(csrc, "vsyn_resample.h")).read()
    define = lambda src, name: re.search(r"#define\s+%s\s+(.+?)\s*(?://.*)?$" % name, src, re.M).group(1)  # noqa: E731
    assert define(rs, "RS_TILE") == "(RS_THREADS * RS_PER_THREAD)" and define(rs, "RS_CHUNK") == "(RS_TILE * RS_TILES)"
    assert int(define(rs, "RS_THREADS")) * int(define(rs, "RS_PER_THREAD")) == nf.RS_TILE and int(define(rs, "RS_TILES")) == nf.RS_TILES
    sp = open(os.path.join(csrc, "vsyn_spectral.h")).read()
    assert int(define(sp, "SPEC_THREADS")) == 256
    assert re.search(r"SPEC_LDS_BUDGET\s*=\s*160u \* 1024u;", sp) and nf.LDS_BYTES == 160 * 1024
    assert "for (uint32_t ft : {16u, 4u, 1u})" in sp and "spec_lds_floats(ft, sp->n_fft, sp->hop_length, sp->n_mels) * 4u <= SPEC_LDS_BUDGET" in sp
    assert "return 3ull * n + spec_span_len(ft, n, hop) + (uint64_t)ft * SPEC_THREADS + (uint64_t)ft * n_mels;" in sp
    assert "return (uint64_t)(ft - 1u) * hop + n;" in sp  # spec_span_len, as nf.mel_lds_floats has it
    pc = open(os.path.join(csrc, "vsyn_pcen.h")).read()
    assert int(define(pc, "PCEN_BLK").rstrip("u")) == nf.PCEN_BLK
