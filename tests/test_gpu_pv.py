"""The phase-vocoder stage on the GPU (include/vorbis_synth_hip.h, "phase vocoder"): every component of every case against the
float64 model of tests/pv_model.py under its derived bound, fed the rows the device reads. Each framing prints its worst |d| /
bound and, since that is the tight float32 rounding by construction, the worst excess over half a float32 unit relative to the
phase terms of the bound; DESIGN.md 6r has the table.

Measured on the MI355X (worst |d| / bound; worst (|d| - 2^-24 |v|) / phase terms): 16 / 4 0.988, <= 0; 64 / 16 0.993, <= 0;
1024 / 256 0.997, 0.00068."""
import ctypes as C

import numpy as np
import pytest

from tests import pv_model as pm

pytestmark = pytest.mark.gpu

FRAMINGS = [(16, 4), (64, 16), (1024, 256)]
RATES = [0.25, 0.5, 0.8, 1.0, 1.25, 2.0 ** (-2.0 / 12.0), 3.0, 200.0]
TAIL = 3  # rows of NaN sentinels behind the output


def fid(e):
    return "%u-%u" % e


@pytest.fixture(scope="module")
def synth():
    import torch
    assert torch.cuda.is_available()
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    yield g
    g.close()


def raw_spec(n_fft, hop):
    """Only n_fft and hop_length are read: everything else stays 0."""
    from parseoggvorbis_amd.binding import SpectralSpec
    return SpectralSpec(n_fft=n_fft, hop_length=hop)


def run_pv(g, n_fft, hop, rows, rates):
    """vsyn_phase_vocoder_device on a batch: rows (list of complex64 [F_g][nb]), rates (list). Returns each segment's rows out
    (complex64 [F_out_g][nb]). The output starts as NaN: the rows behind the last segment's must still be NaN, the input unchanged,
    and seg_rows_out what vsyn_pv_num_rows says."""
    import torch
    nb = n_fft // 2 + 1
    want = [g.lib.vsyn_pv_num_rows(r.shape[0], float(rate)) for r, rate in zip(rows, rates)]
    assert want == [pm.num_rows(r.shape[0], rate) for r, rate in zip(rows, rates)]
    flat = np.concatenate([np.asarray(r, np.complex64).reshape(-1, nb) for r in rows] + [np.zeros((1, nb), np.complex64)])
    d_rows = torch.from_numpy(flat.view(np.float32).copy()).cuda()
    total = sum(want)
    d_out = torch.full((total + TAIL, nb, 2), float("nan"), dtype=torch.float32, device="cuda")
    got = g.phase_vocoder_device(raw_spec(n_fft, hop), [r.shape[0] for r in rows], rates, d_rows.data_ptr(), d_out.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert list(got) == want
    assert np.array_equal(d_rows.cpu().numpy().view(np.uint32), flat.view(np.uint32))  # read only
    out = d_out.cpu().numpy()
    assert np.isnan(out[total:]).all(), "sentinels"
    out = np.ascontiguousarray(out[:total]).view(np.complex64).reshape(total, nb)
    off = np.concatenate([[0], np.cumsum(want)])
    return [out[off[s]:off[s + 1]].copy() for s in range(len(rows))]


# ten segments a call: (F, rate); F_out is 0, 1, exactly 64, 65, 128 / 129 and beyond two block edges; s_t hits integers exactly
# (0.25, 0.5, 1.0), 200 exceeds every F, and the rates differ between the segments of one call
CASES = [(0, 0.8), (1, 1.25), (2, 0.25), (63, 0.5), (64, 1.0), (65, 1.0), (130, 2.0 ** (-2.0 / 12.0)), (130, 0.8), (130, 3.0), (64, 200.0),
         (130, 1.25), (65, 0.5), (63, 0.25), (2, 3.0), (1, 200.0), (130, 1.0), (64, 0.5), (130, 0.25), (65, 0.8), (0, 200.0)]


@pytest.mark.parametrize("entry", FRAMINGS, ids=fid)
def test_stage_against_the_model(synth, entry):
    n, hop = entry
    f_outs = sorted(pm.num_rows(F, r) for F, r in CASES)
    assert {0, 1, 64, 65, 128, 130}.issubset(f_outs) and f_outs[-1] > 192 and {r for _, r in CASES} == set(RATES)
    assert {F for F, _ in CASES} == {0, 1, 2, 63, 64, 65, 130}
    rng = np.random.default_rng(n)
    worst, worst_phase = 0.0, -np.inf
    for call in (CASES[:10], CASES[10:]):
        rows = [pm.random_rows(rng, F, n) for F, _ in call]
        rates = [r for _, r in call]
        got = run_pv(synth, n, hop, rows, rates)
        for s, (F, r) in enumerate(call):
            if got[s].size:
                w, wp = pm.check(got[s], rows[s], r, n, hop, what=(entry, s, F, r))
                worst, worst_phase = max(worst, w), max(worst_phase, wp)
    print("pv %s: worst |d| / bound %.3f, worst (|d| - 2^-24 |v|) / phase terms %.3g" % (fid(entry), worst, worst_phase))
    assert worst > 0.0


@pytest.mark.parametrize("entry", [FRAMINGS[0], FRAMINGS[2]], ids=fid)
def test_same_rows_same_bits(synth, entry):
    """A segment alone, and as segment 0, 3 or 7 of a batch of ten whose other rows are full of 1e30 and whose other rates differ."""
    n, hop = entry
    nb = n // 2 + 1
    rng = np.random.default_rng(n + 1)
    X, rate = pm.random_rows(rng, 130, n), 0.8
    alone = run_pv(synth, n, hop, [X], [rate])[0]
    assert np.isfinite(alone.view(np.float32)).all() and alone.any() and alone.shape[0] == 163
    for pos in (0, 3, 7):
        counts = [5, 0, 3, 70, 9, 2, 64, 6, 1, 3]
        rates = [1.25, 0.5, 3.0, 0.25, 1.0, 200.0, 0.5, 2.0, 0.3, 1.5]
        rows = [np.full((c, nb), 1e30 + 1e30j, np.complex64) for c in counts]
        rows[pos], rates[pos] = X, rate
        got = run_pv(synth, n, hop, rows, rates)[pos]
        assert np.array_equal(got.view(np.uint32), alone.view(np.uint32)), (entry, pos)


def test_signed_zeros_and_a_silent_middle(synth):
    """Row 0 of signed zeros sets acc_0 = atan2 of them: with a unit row behind it at rate 0.5 (alpha = 1/2 at t = 1) the output
    shows the angle. And rows 3..6 of mixed-sign zeros in the middle: the rows behind continue with the model's phases."""
    n, hop = 16, 4
    nb = n // 2 + 1
    z = np.array([complex(-0.0, 0.0), complex(-0.0, -0.0), complex(0.0, 0.0), complex(0.0, -0.0)], np.complex64)
    X = np.ones((2, nb), np.complex64)
    X[0] = z[np.arange(nb) % 4]
    got = run_pv(synth, n, hop, [X], [0.5])[0]
    want = np.arctan2(X[0].imag.astype(np.float64), X[0].real.astype(np.float64))
    assert set(np.abs(want)) == {0.0, np.pi} and (want < 0).any() and (want > 0).any()
    # out[1] = 0.5 * exp(i (A[0] + inc_0)), inc_0 = phi + wrap(0 - A[0] - phi): the model says what that is; pi and -pi must not mix up
    pm.check(got, X, 0.5, n, hop, what="zeros")
    re, im, _ = pm.vocoder(X, 0.5, n, hop)
    assert np.array_equal(np.signbit(got[0].real), np.signbit(re[0])) and np.array_equal(np.signbit(got[0].imag), np.signbit(im[0]))
    rng = np.random.default_rng(3)
    F = 12
    for pat in range(2):
        Xz = pm.random_rows(rng, F, n)
        for f in range(3, 7):
            Xz[f] = z[(np.arange(nb) + f + pat) % 4]
        got = run_pv(synth, n, hop, [Xz], [1.0])[0]
        assert not got[3:7].real.any() and not got[3:7].imag.any()
        assert pm.check(got, Xz, 1.0, n, hop, what=("silent middle", pat))[0] > 0.0


def footprint(F, rate, f, is_nan):
    """The rows of out that step 6 says are non-finite for a NaN (is_nan) or an Inf in row f of the input."""
    i, _ = pm.positions(F, rate)
    hit = (i == f - 1) | (i == f)
    if not is_nan:
        return hit
    if f == 0:
        return np.ones(i.shape, bool)
    out = np.zeros(i.shape, bool)
    if hit.any():
        out[int(np.argmax(hit)):] = True
    return out


@pytest.mark.parametrize("entry", [FRAMINGS[0], FRAMINGS[2]], ids=fid)
def test_nonfinite_footprint(synth, entry):
    """A NaN and an Inf in one bin of row f: at f = 0, at F - 1, and where i_t crosses an output block edge (t = 63 / 64), at a rate
    below 1, at 1 and at one above 2 that steps over rows. Exactly the stated rows of that bin are non-finite; every other bin and
    segment, and the bin's rows in front of them, are bit-equal to the clean run, and behind an Inf the bin is finite again."""
    n, hop = entry
    nb = n // 2 + 1
    rng = np.random.default_rng(n + 2)
    F = 200
    rows = [pm.random_rows(rng, c, n) for c in (4, F, 3)]
    for rate in (0.8, 1.0, 3.0):
        rates = [1.25, rate, 0.5]
        clean = run_pv(synth, n, hop, rows, rates)
        assert all(np.isfinite(c.view(np.float32)).all() for c in clean)
        i, _ = pm.positions(F, rate)
        edge = int(i[63]) if len(i) > 64 else F // 2  # the input row under the last output row of block 0
        stepped = [f for f in range(1, F) if not ((i == f - 1) | (i == f)).any()]
        assert (rate <= 2.0) == (not stepped)
        for f, k in [(0, 1), (F - 1, nb - 1), (edge, 0), (edge + 1, nb // 2), (edge + 2, 3)] + [(s, 2) for s in stepped[:1]]:
            for val in (np.nan, np.inf, -np.inf):
                for part in (0, 1):
                    r2 = [r.copy() for r in rows]
                    x = rows[1][f, k]
                    r2[1][f, k] = complex(val, x.imag) if part == 0 else complex(x.real, val)
                    got = run_pv(synth, n, hop, r2, rates)
                    bad = footprint(F, rate, f, np.isnan(val))
                    assert bad.any() or f in stepped
                    col = got[1][:, k]
                    assert not (np.isfinite(col.real[bad]) & np.isfinite(col.imag[bad])).any(), (entry, rate, f, k, val, part)
                    keep = np.ones(got[1].shape, bool)
                    keep[bad, k] = False
                    if bad.any() and not np.isnan(val):  # behind an Inf the bin is finite again, with the phase its angle left
                        last = len(bad) - int(np.argmax(bad[::-1]))
                        assert np.isfinite(col.real[last:]).all() and np.isfinite(col.imag[last:]).all()
                        keep[last:, k] = False
                    assert np.array_equal(got[1].view(np.uint64)[keep], clean[1].view(np.uint64)[keep]), (entry, rate, f, k, val, part)
                    for s in (0, 2):
                        assert np.array_equal(got[s].view(np.uint32), clean[s].view(np.uint32))


def test_refusals_leave_the_outputs_untouched(synth):
    import torch
    from parseoggvorbis_amd.binding import VsynError
    n, hop, F = 64, 16, 5
    nb = n // 2 + 1
    d_rows = torch.ones((F, nb, 2), dtype=torch.float32, device="cuda")
    d_out = torch.full((F + 2, nb, 2), float("nan"), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    lib, err = synth.lib, C.c_char_p()
    nrows, rates, out_rows = np.array([F], np.uint64), np.array([1.0], np.float64), np.array([77], np.uint64)

    def p(a):
        return None if a is None else C.c_void_p(a.ctypes.data)

    def call(spec=None, S=1, seg_rows=nrows, r=rates, rows=d_rows.data_ptr(), out=d_out.data_ptr()):
        spec = raw_spec(n, hop) if spec is None else spec
        rc = lib.vsyn_phase_vocoder_device(synth.h, C.byref(spec), S, p(seg_rows), p(r), rows, out, p(out_rows), stream, C.byref(err))
        return rc, (err.value or b"").decode()

    refused = [
        ("power of two", dict(spec=raw_spec(1102, 441))),
        ("n_fft", dict(spec=raw_spec(8, 2))),
        ("n_fft", dict(spec=raw_spec(16384, 4096))),
        ("hop_length", dict(spec=raw_spec(n, 0))),
        ("rate", dict(r=np.array([0.0]))),
        ("rate", dict(r=np.array([-1.0]))),
        ("rate", dict(r=np.array([np.nan]))),
        ("rate", dict(r=np.array([np.inf]))),
        ("too many rows", dict(seg_rows=np.array([2 ** 30], np.uint64))),
        ("too many rows out", dict(r=np.array([1e-9]))),
        ("seg_rows", dict(seg_rows=None)),
        ("rates", dict(r=None)),
        ("NULL", dict(rows=None)),
        ("NULL", dict(out=None)),
        ("too many segments", dict(S=65536, seg_rows=np.zeros(65536, np.uint64), r=np.ones(65536))),
    ]
    for word, kw in refused:
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (word, rc, msg)
    assert lib.vsyn_phase_vocoder_device(synth.h, None, 0, None, None, None, None, None, stream, C.byref(err)) != 0
    with pytest.raises(VsynError):
        synth.phase_vocoder_device(raw_spec(n, hop), [F], [0.0], d_rows.data_ptr(), d_out.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.isnan(d_out.cpu().numpy()).all() and out_rows[0] == 77
    rc, msg = call()  # and the same call with nothing wrong runs
    assert rc == 0, msg
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.isfinite(out[:F]).all() and np.isnan(out[F:]).all() and out_rows[0] == F
