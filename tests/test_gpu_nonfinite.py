"""What an Inf or NaN value does in every stage that reads PCM or rows, on the device, held to the rule that the header states and
tests/test_nonfinite_cpu.py settles on the float64 models: step 8 of "spectral features", step 6 of "linear spectra", step 3 of
"resampling", step 5 of "spectral post-processing", rule 7 of "PCEN" and the VSYN_PCM_S16 line of include/vorbis_synth_hip.h.

One shape throughout (tests/nonfinite_cases.py): three segments of seeded noise of different lengths, two channels where the entry
takes channels, every plane NaN behind its segment's frames, every output a NaN sentinel first; a clean run and a dirty run through
the stage's _device entry on one handle, the dirty batch being the clean one with NaN, +Inf or -Inf in one channel of segment 1
(t = 0, t = T - 1, a sample that the last frame of a workgroup tile and the first of the next both cover, a sample behind the last
whole frame, and +Inf beside -Inf in one frame). Outside the footprint, which the helper computes from the header's formulas, the
dirty output has the clean one's bits, the offsets, row counts and sentinels included; inside it no value is finite; the status is
clean. No tolerance anywhere: every comparison is of bits.

What the kernels need for it: floors and a clamp that keep a NaN (a comparison, where fmaxf returns the floor: a frame with a NaN
sample came back from log_mel, mel_db, mfcc and lin_db as the floor's value, a silent frame) and a segment maximum fed from finite dB
values only (a +Inf won it and the clamp wrote +Inf over the whole segment). The resampler reads K4 taps, K rounded up to a multiple
of 4, whose padding is +0: its footprint is by K4, as the header now says. Measured on the MI355X: the module's 34 tests take 1.8 s."""
import ctypes as C

import numpy as np
import pytest

from tests import nonfinite_cases as nf
from tests import resample_model as rm
from tests import spectral_model as sm

pytestmark = pytest.mark.gpu

SHAPE_ID = lambda s: "n%d_h%d_w%d_%s" % (s[0], s[1], s[2], "c" if s[3] else "nc")  # noqa: E731


@pytest.fixture(scope="module")
def spec_mod():
    import torch
    assert torch.cuda.is_available()
    from parseoggvorbis_amd import spectral
    return spectral


@pytest.fixture(scope="module")
def synth():
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import fixture_like_spec
    g = Synth(fixture_like_spec(2), device=0, max_streams=4)
    yield g
    g.close()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _clean_status(g):
    import torch
    torch.cuda.synchronize()
    assert g.sync_status(_stream())[0] == 0


def _spectral(g, spec, pcm, frames, rates=None):
    """vsyn_spectral_device: (rows float32 [S fmax + 1][dim] over a NaN sentinel, offsets [S + 1])."""
    import torch
    from parseoggvorbis_amd import spectral
    S, Cn, plane = pcm.shape
    dim = spectral.spec_dim(spec)
    fmax = sm.num_frames(plane, spec.n_fft, spec.hop_length, bool(spec.options & spectral.OPT_CENTER))
    d_pcm = torch.from_numpy(pcm).cuda()
    d_frames = torch.from_numpy(np.asarray(frames, np.int32)).cuda()
    d_rows = torch.full((S * fmax + 1, dim), float("nan"), dtype=torch.float32, device="cuda")
    d_off = torch.full((S + 1,), -1, dtype=torch.int64, device="cuda")
    g.spectral_device(spec, [nf.MEL_SR] * S if rates is None else rates, d_pcm.data_ptr(), plane, Cn, d_frames.data_ptr(), d_rows.data_ptr(),
                      d_off.data_ptr(), _stream())
    torch.cuda.synchronize()
    return d_rows.cpu().numpy(), d_off.cpu().numpy()


def _spectral_shape(g, spec_mod, shape, kinds, n_mels=None):
    n, hop, win, center, lengths, tile = shape
    T = lengths[nf.DIRTY_SEG]
    pcm, frames = nf.pcm_batch(lengths, 2, seed=n + hop)
    pos = nf.spectral_positions(T, n, hop, win, center, tile)
    want_off = np.concatenate([[0], np.cumsum([sm.num_frames(t, n, hop, center) for t in lengths])])
    for kind, kw in kinds:
        extra = dict(kw, n_mels=n_mels) if n_mels else kw
        spec = spec_mod.spectral_spec(kind, n_fft=n, hop_length=hop, win_length=win, center=center, **extra)
        if n_mels is None:
            assert g.lib.vsyn_spectral_lin_tile(C.byref(spec)) == tile
        clean, off = _spectral(g, spec, pcm, frames)
        assert np.array_equal(off, want_off)
        assert np.isfinite(clean[:off[3]]).all() and np.isnan(clean[off[3]:]).all()  # what lies behind a segment's frames is never read
        for name, vname in nf.cases(pos):
            what = (SHAPE_ID(shape), kind, kw, name, vname)
            dirty, off2 = _spectral(g, spec, nf.dirtied(pcm, nf.writes_of(name, pos[name], vname)), frames)
            assert np.array_equal(off2, off), what
            fp = nf.spectral_footprint(pos[name], T, n, hop, win, center)
            if name == "behind" or (name == "first" and not center and win < n):
                assert not fp.any(), what  # no frame's support holds the sample: the whole output is the clean one
            else:
                assert fp.any(), what
            hit = np.zeros(clean.shape[0], bool)
            hit[off[1] + np.flatnonzero(fp)] = True
            cols = clean.shape[1] // 2 if kind == "stft" else clean.shape[1]
            nf.assert_footprint(clean, dirty, np.repeat(hit[:, None], cols, axis=1), what, complex_values=kind == "stft")
    _clean_status(g)


@pytest.mark.parametrize("shape", nf.LIN_SHAPES, ids=SHAPE_ID)
def test_linear_kinds(spec_mod, synth, shape):
    """lin_power at both powers, lin_db and stft: the FFT kernel with 32 frames and with one frame per tile, the direct kernel with 8
    frames and with one, and a window shorter than n_fft, where a sample inside the frame but outside the window's support leaves the
    frame's bits alone. For stft a value is the complex bin."""
    _spectral_shape(synth, spec_mod, shape, nf.LIN_KINDS)


@pytest.mark.parametrize("shape", nf.MEL_SHAPES, ids=SHAPE_ID)
def test_mel_kinds(spec_mod, synth, shape):
    """mel_power, log_mel, mel_db and mfcc with 8 bands at one shape for each tile the mel kernel takes, 16, 4 and 1 frames, and at
    the 16-frame tile without centring as well (pad = 0, a tail that is loaded into the tile's span and belongs to no frame, t = 0 a
    frame's own sample), once with win_length < n_fft (woff > 0: t = 0 lies in frame 0 and outside its support)."""
    assert nf.mel_tile(shape[0], shape[1], nf.N_MELS) == shape[5]
    _spectral_shape(synth, spec_mod, shape, nf.MEL_KINDS, n_mels=nf.N_MELS)


@pytest.mark.parametrize("kind,n,hop,extra,center", nf.TOP_DB_SHAPES, ids=nf.TOP_DB_IDS)
def test_top_db(spec_mod, synth, kind, n, hop, extra, center):
    """top_db in {0, 80, 20}: a dB value that is not finite takes no part in the segment's maximum and the clamp leaves it as it is. So
    outside the footprint the rows are, bit for bit, the float32 clamp of the device's own top_db = 0 rows of the clean signal against
    their maximum over the rows outside the footprint (for mfcc: the float32 fma chain of the DCT over those); once with the clean
    maximum inside the footprint and once outside it. Segments 0 and 2 are the clean run's at that top_db."""
    lengths = nf.TOP_DB_LENGTHS
    T = lengths[nf.DIRTY_SEG]
    pcm, frames = nf.pcm_batch(lengths, 2, seed=5, burst=nf.TOP_DB_BURST)
    db_kind = "lin_db" if kind == "lin_db" else "mel_db"
    kw = {k: v for k, v in extra.items() if k != "n_mfcc"}
    rows0, off = _spectral(synth, spec_mod.spectral_spec(db_kind, n_fft=n, hop_length=hop, center=center, top_db=None, **kw), pcm, frames)
    D0 = rows0[off[1]:off[2]]
    assert np.isfinite(D0).all() and float(D0.max() - D0.min()) > 80.0
    row_max = int(np.argmax(D0.max(axis=1)))
    for top_db in nf.TOP_DB:
        spec = spec_mod.spectral_spec(kind, n_fft=n, hop_length=hop, center=center, top_db=top_db or None, **extra)
        clean, off1 = _spectral(synth, spec, pcm, frames)
        assert np.array_equal(off1, off)
        for where, s in (("inside", nf.TOP_DB_BURST[0] + nf.TOP_DB_BURST[1] // 2), ("outside", 0)):
            fp = nf.spectral_footprint([s], T, n, hop, n, center)
            assert fp[row_max] == (where == "inside") and fp.any() and not fp.all()
            want = nf.clamp32(D0, ~fp, top_db)
            if top_db:
                assert (want[~fp] > D0[~fp]).any()  # the clamp is at work in the rows that are compared
            if kind == "mfcc":
                want = nf.mfcc32(want, nf.N_MFCC)
            for vname, v in nf.VALUES.items():
                what = (kind, n, top_db, where, vname)
                dirty, off2 = _spectral(synth, spec, nf.dirtied(pcm, [(s, v)]), frames)
                assert np.array_equal(off2, off), what
                got = dirty[off[1]:off[2]]
                bad = nf.bits(got[~fp]) != nf.bits(want[~fp])
                assert not bad.any(), (what, int(bad.sum()), got[~fp][bad][:4], want[~fp][bad][:4])
                assert not np.isfinite(got[fp]).any(), what
                other = np.ones(clean.shape[0], bool)
                other[off[1]:off[2]] = False
                assert np.array_equal(nf.bits(dirty[other]), nf.bits(clean[other])), what
    _clean_status(synth)


def _resample(g, pcm, frames, r_in, r_out):
    import torch
    S, Cn, plane = pcm.shape
    out_plane = rm.num_frames(r_in, r_out, plane) + 3
    d_pcm = torch.from_numpy(pcm).cuda()
    d_frames = torch.from_numpy(np.asarray(frames, np.int32)).cuda()
    d_out = torch.full((S, Cn, out_plane), float("nan"), dtype=torch.float32, device="cuda")
    d_of = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    g.resample_device([r_in] * S, r_out, d_pcm.data_ptr(), plane, Cn, d_frames.data_ptr(), d_out.data_ptr(), out_plane, d_of.data_ptr(), _stream())
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_of.cpu().numpy()


@pytest.mark.parametrize("r_in,r_out,lengths", nf.RS_SHAPES, ids=["%d_%d" % s[:2] for s in nf.RS_SHAPES])
def test_resample(synth, r_in, r_out, lengths):
    """2 -> 1, 1 -> 2 and 3 -> 2 (table in LDS) and 11025 -> 32000 (table in global memory), every one a pair with padded taps: output
    j is not finite exactly when one of its K4 taps is (step 3), in the dirty channel alone; both kernel variants are held to the same
    footprint and to their own clean bits, and t = 0 and t = T - 1 take the guarded loads of either. That the two variants give each
    other's bits is not asserted: a rate pair selects one variant by its table's size and nothing forces the other."""
    T = lengths[nf.DIRTY_SEG]
    pcm, frames = nf.pcm_batch(lengths, 2, seed=r_in % 1000, plane=max(lengths) + 5)  # an odd plane: channel 1 is not 16-byte aligned
    pos = nf.resample_positions(T, r_in, r_out)
    clean, of = _resample(synth, pcm, frames, r_in, r_out)
    assert of.tolist() == [rm.num_frames(r_in, r_out, t) for t in lengths]
    for g_ in range(3):
        assert np.isfinite(clean[g_, :, :of[g_]]).all() and np.isnan(clean[g_, :, of[g_]:]).all()
    for ch in (0, 1):
        for name, vname in nf.cases(pos):
            what = (r_in, r_out, ch, name, vname)
            dirty, of2 = _resample(synth, nf.dirtied(pcm, nf.writes_of(name, pos[name], vname), ch=ch), frames, r_in, r_out)
            assert np.array_equal(of2, of), what
            fp = nf.resample_footprint(pos[name], T, r_in, r_out)
            assert fp.any() and not fp.all()
            hit = np.zeros(clean.shape, bool)
            hit[nf.DIRTY_SEG, ch, :of[1]] = fp
            nf.assert_footprint(clean, dirty, hit, what)
    _clean_status(synth)


def _pcen(g, spec_mod, rows, seg_rows, in_place, **kw):
    import torch
    n, D = rows.shape[0] - 3, rows.shape[1]
    d_in = torch.from_numpy(rows).cuda()
    d_out = d_in if in_place else torch.full((n + 3, D), float("nan"), dtype=torch.float32, device="cuda")
    g.spectral_pcen_device(spec_mod.pcen_spec(**kw), D, seg_rows, [nf.PCEN_KW["sr"]] * len(seg_rows), nf.PCEN_KW["hop_length"], d_in.data_ptr(),
                           d_out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("extra", [dict(), dict(bias=0.0), dict(power=0.0), dict(gain=0.0)], ids=["default", "bias0", "power0", "gain0"])
def test_pcen(spec_mod, synth, extra):
    """Segments of 3, 700 and 41 rows, the value in row 0, in the last row of a 64-row block of the scan, in the first row of the next and
    in the last row of segment 1. A NaN and a -Inf: that column is not finite from the row on; rows before it, the other columns and the
    other segments keep their bits. A +Inf (rule 7): its row is not finite, and with gain > 0 the rows behind it are the 0 that a gain
    G = 0 gives, because M stays +Inf; with gain = 0 the column is NaN from the row on. In place and out of place give the same bits."""
    F, D, d = nf.PCEN_ROWS[1], nf.PCEN_D, nf.PCEN_COL
    rows, first = nf.rows_batch(nf.PCEN_ROWS, D, seed=3, positive=True)
    clean = _pcen(synth, spec_mod, rows, nf.PCEN_ROWS, False, **extra)
    assert np.isfinite(clean[:-3]).all() and np.isnan(clean[-3:]).all()
    for f in nf.PCEN_DIRTY_ROWS:
        for vname, v in nf.VALUES.items():
            what = (extra, f, vname)
            bad = rows.copy()
            bad[first[1] + f, d] = v
            dirty = _pcen(synth, spec_mod, bad, nf.PCEN_ROWS, False, **extra)
            assert np.array_equal(nf.bits(_pcen(synth, spec_mod, bad, nf.PCEN_ROWS, True, **extra)), nf.bits(dirty)), what
            hit = np.zeros(clean.shape, bool)
            if vname == "+inf" and extra.get("gain", 1.0) > 0:
                own, forced = nf.pcen_plus_inf(f, d, F, D)
                hit[first[1]:first[2]] = own
                zero = np.zeros(clean.shape, bool)
                zero[first[1]:first[2]] = forced
                assert (nf.bits(dirty[zero]) == 0).all(), what
                dirty = np.where(zero, clean, dirty)  # the forced rows are settled; the rest goes through the one comparison
            else:
                hit[first[1]:first[2]] = nf.pcen_footprint(f, d, F, D)
            nf.assert_footprint(clean, dirty, hit, what)
    _clean_status(synth)


def _post(g, post, rows, seg_rows):
    import torch
    n, D = rows.shape[0] - 3, rows.shape[1]
    dout = D * (1 + post.order)
    d_in = torch.from_numpy(rows).cuda()
    d_out = torch.full((n + 3, dout), float("nan"), dtype=torch.float32, device="cuda")
    g.spectral_post_device(post, D, seg_rows, d_in.data_ptr(), d_out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("order", nf.POST_ORDERS)
@pytest.mark.parametrize("width", nf.POST_WIDTHS)
def test_post_stage(spec_mod, synth, order, width):
    """Deltas alone, and with the segment's own mean and mean / variance: the value in an interior row, in row h, whose delta the h edge
    rows repeat, and in the last interior row. Y[f][d] and the delta rows that read row f are not finite; with VSYN_POST_STATS_SEGMENT
    the whole column of that segment is, in every block it feeds (d, D + d, 2 D + d); other columns and segments keep their bits."""
    F, D, d = nf.POST_ROWS[1], nf.POST_D, nf.POST_COL
    rows, first = nf.rows_batch(nf.POST_ROWS, D, seed=4, positive=False)
    for norm in (None, "mean", "mean_var"):
        post = spec_mod.post_spec(D, delta=order, delta_width=width, normalize=norm)[0]
        clean = _post(synth, post, rows, nf.POST_ROWS)
        assert np.isfinite(clean[:-3]).all() and np.isnan(clean[-3:]).all()
        for f in nf.post_dirty_rows(F, width):
            for vname, v in nf.VALUES.items():
                bad = rows.copy()
                bad[first[1] + f, d] = v
                hit = np.zeros(clean.shape, bool)
                hit[first[1]:first[2]] = nf.post_footprint(f, d, F, D, order, width, norm is not None)
                nf.assert_footprint(clean, _post(synth, post, bad, nf.POST_ROWS), hit, (order, width, norm, f, vname))
    _clean_status(synth)


def _submitted(spec, streams, packets, seed):
    """A handle whose last submit (device entry) has `streams` segments, and their frames."""
    import torch
    from parseoggvorbis_amd.binding import Synth
    from tests.workloads import synth_batch
    b = synth_batch(spec, streams, packets, pattern="long", seed=seed)
    g = Synth(spec, device=0, max_streams=streams)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    P, S, plane = len(b["packets"]), streams, b["plane_stride"]
    bufs = [dev(b[k]) for k in ("packets", "segments", "ys", "residue")]
    d_pcm = torch.zeros((S, spec.channels, plane), device="cuda")
    d_emit = torch.zeros(P, dtype=torch.int32, device="cuda")
    g.submit_device(P, bufs[0].data_ptr(), S, bufs[1].data_ptr(), packets, bufs[2].data_ptr(), bufs[3].data_ptr(), d_pcm.data_ptr(), plane,
                    d_emit.data_ptr(), None, 0, _stream())
    torch.cuda.synchronize()
    assert g.sync_status(_stream())[0] == 0
    return g, d_emit.cpu().numpy().reshape(S, packets).sum(axis=1).astype(np.int64)


@pytest.mark.parametrize("channels,path", [(2, "aligned"), (2, "odd_stride"), (2, "offset"), (1, "mono")])
def test_int16_of_nan_and_inf_device(channels, path):
    """vsyn_pcm_interleave_device, VSYN_PCM_S16, on planes of the caller's: the vectorised stereo path (a 16-byte aligned pointer and a
    plane_stride that is a multiple of 4), the generic path through an odd plane_stride, through a pointer one float off, and for mono.
    NaN, +-Inf, +-1, +-65536 and the largest finite floats give the header's values at every site, and every other sample numpy's
    restatement of the line; the float32 form passes the same values through with their bits."""
    import torch
    from parseoggvorbis_amd.binding import VSYN_PCM_F32, VSYN_PCM_S16
    from tests.workloads import fixture_like_spec
    g, emitted = _submitted(fixture_like_spec(channels), 3, 4, seed=21)
    S, k = 3, len(nf.S16_INPUTS)
    frames = int(emitted.min())
    assert (emitted == frames).all() and frames > 4 * k
    plane = (frames // 4 + 2) * 4 + (path == "odd_stride")
    assert plane > frames and (plane % 2 == 1 if path == "odd_stride" else plane % 4 == 0)
    rng = np.random.default_rng(6)
    x = np.full((S, channels, plane), np.nan, np.float32)
    x[:, :, :frames] = (1.5 * rng.standard_normal((S, channels, frames))).astype(np.float32)  # some of it clamps
    x[1, channels - 1, :k] = nf.S16_INPUTS              # whole groups of four frames: the vectorised path where it is taken
    x[1, 0, frames - k:frames] = nf.S16_INPUTS[::-1]    # and the segment's last frames, the ragged group among them
    x[2, 0, 5:5 + k] = -nf.S16_INPUTS
    off = 1 if path == "offset" else 0
    buf = torch.full((x.size + 8,), float("nan"), dtype=torch.float32, device="cuda")
    buf[off:off + x.size] = torch.from_numpy(x.reshape(-1)).cuda()
    assert buf.data_ptr() % 16 == 0
    d_s16 = torch.full((S, frames + 2, channels), 12345, dtype=torch.int16, device="cuda")
    d_f32 = torch.full((S, frames + 2, channels), 7.0, dtype=torch.float32, device="cuda")
    d_frames = torch.zeros(S, dtype=torch.int32, device="cuda")
    g.pcm_interleave_device(VSYN_PCM_S16, buf.data_ptr() + 4 * off, plane, d_s16.data_ptr(), frames + 2, d_frames.data_ptr(), _stream())
    g.pcm_interleave_device(VSYN_PCM_F32, buf.data_ptr() + 4 * off, plane, d_f32.data_ptr(), frames + 2, None, _stream())
    _clean_status(g)
    s16, f32 = d_s16.cpu().numpy(), d_f32.cpu().numpy()
    assert d_frames.cpu().numpy().tolist() == [frames] * S
    want = np.transpose(x[:, :, :frames], (0, 2, 1))
    assert np.array_equal(s16[:, :frames], nf.s16(want)) and (s16[:, frames:] == 12345).all()
    assert np.array_equal(nf.bits(f32[:, :frames]), nf.bits(want)) and (f32[:, frames:] == 7.0).all()
    assert np.array_equal(s16[1, :k, channels - 1], nf.S16_WANT) and np.array_equal(s16[1, frames - k:frames, 0], nf.S16_WANT[::-1])
    g.close()


@pytest.mark.parametrize("bs0,bs1", [(256, 2048), (128, 1024)], ids=["256_2048", "128_1024"])
def test_host_chain_with_a_nan_residue(spec_mod, bs0, bs1):
    """Through the host forms: a submit_host batch of 2 streams x 12 long packets, KEEP_PCM, with one NaN in one residue value of stream
    1 (256/2048 takes the fused long-block kernel, 128/1024 the generic one). Against the CPU oracle on the same arrays: the PCM frames
    that are not finite are the oracle's, stream 0 has the bits of the clean submit, and every finite frame is inside the 1e-5 gate of
    the synthesis tests. vsyn_pcm_fetch_host and vsyn_pcm_resample_host convert those frames to int16 as the header's line says. Then
    vsyn_pcm_spectral_host (log_mel, lin_db) has the bits of vsyn_spectral_device on the fetched PCM. Last, the same batch with its
    residue scaled up, so that the two host sites of the int16 conversion also see products far outside the range and products that
    overflow to +-Inf. A PCM sample that is itself +-Inf reaches them only if the synthesis overflows, which is not forced here: +-Inf
    samples are converted through vsyn_pcm_interleave_device alone (test_int16_of_nan_and_inf_device)."""
    import torch
    from oracle.oracle_binding import OracleSynth
    from parseoggvorbis_amd.binding import Synth, VSYN_PCM_F32, VSYN_PCM_S16, VSYN_SUBMIT_KEEP_PCM
    from tests.workloads import fixture_like_spec, synth_batch
    spec = fixture_like_spec(2, bs0, bs1)
    b = synth_batch(spec, streams=2, packets_per_stream=12, pattern="long", seed=31)
    S, plane, n2 = 2, b["plane_stride"], bs1 // 2
    res = b["residue"].copy()
    res[int(b["segments"][1]["residue_off"]) + 5 * 2 * n2 + n2 // 3] = np.nan  # stream 1, packet 5, channel 0
    args = lambda r: (b["packets"], b["segments"], b["ys"], r, plane)  # noqa: E731
    g = Synth(spec, device=0, max_streams=2)
    clean = g.submit_host(*args(b["residue"]))
    g.reset()
    dirty = g.submit_host(*args(res))
    want = OracleSynth(spec, 2).submit_host(*args(res))
    assert clean["rc"] == 0 and dirty["rc"] == 0 and want["rc"] == 0 and dirty["flags"] == 0
    assert np.array_equal(dirty["emit_len"], want["emit_len"]) and np.array_equal(dirty["emit_len"], clean["emit_len"])
    frames = dirty["emit_len"].reshape(S, 12).sum(axis=1).astype(np.int64)
    bad = ~np.isfinite(dirty["pcm"])
    assert np.array_equal(bad, ~np.isfinite(want["pcm"])), (int(bad.sum()), int((~np.isfinite(want["pcm"])).sum()))
    assert bad[1].any() and not bad[0].any() and not bad[1].all()
    assert np.array_equal(nf.bits(dirty["pcm"][0]), nf.bits(clean["pcm"][0]))
    scale = float(np.abs(want["pcm"][~bad]).max())
    assert float(np.abs(dirty["pcm"][~bad] - want["pcm"][~bad]).max()) < 1e-5 * max(1.0, scale)
    # the host forms of the int16 conversion on the kept PCM
    g.reset()
    kept = g.submit_host(*args(res), flags=VSYN_SUBMIT_KEEP_PCM)
    assert kept["rc"] == 0
    stride = int(frames.max())
    f32, fr = g.pcm_fetch_host(VSYN_PCM_F32, S, stride)
    s16, fr2 = g.pcm_fetch_host(VSYN_PCM_S16, S, stride)
    assert fr.tolist() == frames.tolist() == fr2.tolist()
    for gi in range(S):
        assert np.array_equal(nf.bits(f32[gi, :frames[gi]]), nf.bits(dirty["pcm"][gi, :, :frames[gi]].T))
        assert np.array_equal(s16[gi, :frames[gi]], nf.s16(f32[gi, :frames[gi]]))
    assert (s16[1][~np.isfinite(f32[1])] == -32768).all() and not np.isfinite(f32[1]).all()
    for rates, out in (([16000, 16000], 16000), ([16000, 16000], 8000)):
        rf, n_out = g.pcm_resample_host(rates, out, VSYN_PCM_F32)
        rs, n_out2 = g.pcm_resample_host(rates, out, VSYN_PCM_S16)
        assert np.array_equal(n_out, n_out2)
        for gi in range(S):
            m = int(n_out[gi])
            assert np.array_equal(rs[gi, :m], nf.s16(rf[gi, :, :m].T)), (out, gi)
        assert not np.isfinite(rf[1]).all() and np.isfinite(rf[0]).all()
    # the spectral host form against the device entry on the fetched PCM
    planar = np.full((S, 2, stride + 3), np.nan, np.float32)
    for gi in range(S):
        planar[gi, :, :frames[gi]] = f32[gi, :frames[gi]].T
    for kind, kw in (("log_mel", dict(n_fft=400, hop_length=160, n_mels=nf.N_MELS)), ("lin_db", dict(n_fft=1024, hop_length=256))):
        s = spec_mod.spectral_spec(kind, **kw)
        r = g.pcm_spectral_host(s, [nf.MEL_SR] * S)
        rows, off = _spectral(g, s, planar, frames.astype(np.int32))
        assert r["rc"] == 0 and r["seg_rows"].tolist() == np.diff(off).tolist()
        assert np.array_equal(nf.bits(r["rows"]), nf.bits(rows[:off[S]])), kind
        seg1 = rows[off[1]:off[2]]
        assert not np.isfinite(seg1).all() and np.isfinite(seg1).any() and np.isfinite(rows[:off[1]]).all()
    # large values at the same host sites (a NaN residue gives NaN frames and ordinary samples only): stream 0's residue times 1e6,
    # so that every product x * 32768 lies far outside the int16 range, and stream 1's times 3e36 (PCM near 1e34 .. 1e35), so that it overflows float32 to +-Inf
    big = b["residue"].copy()
    o1 = int(b["segments"][1]["residue_off"])
    big[:o1] *= np.float32(1e6)
    big[o1:] *= np.float32(3e36)
    g.reset()
    assert g.submit_host(*args(big), flags=VSYN_SUBMIT_KEEP_PCM)["rc"] == 0
    f32, fr = g.pcm_fetch_host(VSYN_PCM_F32, S, stride)
    s16, _ = g.pcm_fetch_host(VSYN_PCM_S16, S, stride)
    assert fr.tolist() == frames.tolist()
    x0, x1 = f32[0, :frames[0]], f32[1, :frames[1]]
    assert np.isfinite(x0).all() and float(np.mean(np.abs(x0) > 2.0)) > 0.5
    with np.errstate(over="ignore"):
        assert np.isinf(x1[np.isfinite(x1)] * np.float32(32768.0)).any()
    for gi in range(S):
        got, want16 = s16[gi, :frames[gi]], nf.s16(f32[gi, :frames[gi]])
        assert np.array_equal(got, want16), gi
        assert (got == 32767).any() and (got == -32768).any()
    rf, n_out = g.pcm_resample_host([16000, 16000], 8000, VSYN_PCM_F32)
    rs, _ = g.pcm_resample_host([16000, 16000], 8000, VSYN_PCM_S16)
    for gi in range(S):
        m = int(n_out[gi])
        assert np.array_equal(rs[gi, :m], nf.s16(rf[gi, :, :m].T)), gi
        assert (rs[gi, :m] == 32767).any() and (rs[gi, :m] == -32768).any()
    _clean_status(g)
    g.close()
