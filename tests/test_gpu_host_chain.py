"""What the host entries behind the last host submit do around their work, pinned as it is: vsyn_pcm_resample_host,
vsyn_pcm_condition_host, vsyn_pcm_trim_host, vsyn_pcm_split_host, vsyn_pcm_split_intervals_host, vsyn_pcm_spectral_host,
vsyn_pcm_spectral_post_host, vsyn_pcm_resample_spectral_host, vsyn_pcm_cond_spectral_host, vsyn_pcm_trim_spectral_host,
vsyn_pcm_split_spectral_host, vsyn_pcm_pitch_host and vsyn_pcm_fdesc_host.

    refusals      REFUSED below: per entry and fault, which outputs a refused call has written (the rest keep the caller's bytes), and
                  that the call after it gives the bits of the call before it.
    nested forms  an entry with a stage passed as NULL gives the bits of the entry without that stage.
    short rows    a segment gated below the delta width loses its rows alone; ungated, the call is refused.

Nothing here is a tolerance: every comparison is of bytes, and the tables are literals.
"""
import ctypes as C
import types

import numpy as np
import pytest

from tests.test_gpu_condition import A, _cond, mods  # noqa: F401
from tests.test_gpu_trim import _trim

pytestmark = pytest.mark.gpu

K = 77  # what every output holds before a call
RATE, OUT = 44100, 22050
KEPT, ZERO, GOOD, UNGATED, RESET = "kept", "zero", "good", "ungated", "reset"

# entry -> (channels of out: 0 = the handle's, outputs in the caller's memory, the rates it can run at)
ENTRIES = {
    "resample": (0, ("out", "frames"), (OUT,)),
    "condition": (1, ("out", "frames", "peaks"), (0, OUT)),
    "trim": (1, ("out", "frames", "bounds", "peaks", "refs"), (0, OUT)),
    "split": (1, ("out", "frames", "counts", "iv", "peaks", "refs"), (0, OUT)),
    "split_intervals": (1, ("frames", "counts", "iv", "refs"), (0, OUT)),
    "spectral": (1, ("rows", "seg_rows", "status"), (0,)),
    "spectral_post": (1, ("rows", "seg_rows", "status"), (0, OUT)),
    "resample_spectral": (1, ("rows", "seg_rows", "status"), (OUT,)),
    "cond_spectral": (1, ("rows", "seg_rows", "peaks", "status"), (0, OUT)),
    "trim_spectral": (1, ("rows", "seg_rows", "bounds", "peaks", "refs", "status"), (0, OUT)),
    "split_spectral": (1, ("rows", "seg_rows", "frames", "counts", "iv", "peaks", "refs", "status"), (0, OUT)),
    "pitch": (1, ("rows", "seg_rows", "refused", "status"), (0, OUT)),
    "fdesc": (1, ("rows", "seg_rows", "refused", "status"), (0, OUT)),
}

# What a refused call leaves in each output; an output not named keeps the caller's bytes. ZERO: cleared over the num_segments of
# the call; GOOD: what the accepted call writes there; UNGATED: the frames in front of the gate; RESET: the status of a call that
# found nothing. Faults: no host submit on the handle yet; num_segments one above the submit's; a format that is neither; frames_out
# (seg_rows, for an entry that returns rows) NULL; out_stride_frames one below the longest segment; rows_capacity one below the
# total; intervals_stride one below vsyn_pcm_split_max_intervals of the longest segment.
_NOT_YET = dict(peaks=ZERO)
_PCM = dict(no_submit=_NOT_YET, segments=_NOT_YET, format={}, null={})
_ROWS0 = dict(seg_rows=ZERO, status=RESET)
_ROWS = dict(no_submit=_ROWS0, segments=_ROWS0, null=dict(status=RESET), capacity=dict(seg_rows=GOOD, status=RESET))
_ROWS0_PEAKS = dict(_ROWS0, peaks=ZERO)
_ROWS0_SPLIT = dict(_ROWS0_PEAKS, refs=ZERO)
_ROWS0_TRIM = dict(_ROWS0_SPLIT, bounds=ZERO)
_ROWS0_REFUSED = dict(_ROWS0, refused=ZERO)
_ROWS_REFUSED = dict(no_submit=_ROWS0_REFUSED, segments=_ROWS0_REFUSED, null=dict(status=RESET),
                     capacity=dict(seg_rows=GOOD, refused=ZERO, status=RESET))
REFUSED = {
    "resample": dict(no_submit={}, segments={}, format={}, null={}, stride=dict(frames=GOOD)),
    "condition": dict(_PCM, stride=dict(frames=GOOD, peaks=ZERO)),
    "trim": dict(_PCM, stride=dict(frames=UNGATED, peaks=ZERO)),
    "split": dict(_PCM, stride=dict(frames=UNGATED, peaks=ZERO), ivs=dict(frames=UNGATED, peaks=ZERO)),
    "split_intervals": dict(no_submit={}, segments={}, null={}, ivs=dict(frames=GOOD)),
    "spectral": _ROWS,
    "spectral_post": _ROWS,
    "resample_spectral": _ROWS,
    "cond_spectral": dict(no_submit=_ROWS0_PEAKS, segments=_ROWS0_PEAKS, null=dict(status=RESET),
                          capacity=dict(seg_rows=GOOD, peaks=ZERO, status=RESET)),
    "trim_spectral": dict(no_submit=_ROWS0_TRIM, segments=_ROWS0_TRIM, null=dict(status=RESET),
                          capacity=dict(seg_rows=GOOD, bounds=GOOD, refs=GOOD, peaks=ZERO, status=RESET)),
    "split_spectral": dict(no_submit=_ROWS0_SPLIT, segments=_ROWS0_SPLIT, null=dict(status=RESET), ivs=_ROWS0_SPLIT,
                           capacity=dict(seg_rows=GOOD, frames=GOOD, counts=GOOD, iv=GOOD, refs=GOOD, peaks=ZERO, status=RESET)),
    "pitch": _ROWS_REFUSED,
    "fdesc": _ROWS_REFUSED,
}


class Chain:
    """One handle and the specs every entry is driven with, through raw lib.vsyn_* calls on outputs filled with K."""

    def __init__(self, spectral):
        from parseoggvorbis_amd.binding import SpectralPost, Synth
        from parseoggvorbis_amd.frame_descriptors import fdesc_spec
        from parseoggvorbis_amd.pitch import pitch_spec
        from tests.workloads import fixture_like_spec, synth_batch
        spec = fixture_like_spec(2)
        self.batch = synth_batch(spec, streams=3, packets_per_stream=12, pattern="mixed", seed=31)
        self.S = len(self.batch["segments"])
        self.g = Synth(spec, device=0, max_streams=4)
        self.lib = self.g.lib
        self.gate = _trim(3.0, 64, 16)  # 3 dB under the loudest frame: pauses inside
        self.cond = _cond(True, A)
        self.spec = spectral.spectral_spec(kind="log_mel", n_fft=400, hop_length=160, n_mels=40)
        self.post = SpectralPost(1, 3, 2, 0, 1e-5, None, None)
        self.pitch = pitch_spec(80.0, 2000.0, frame_length=400, hop_length=160)
        self.fdesc = fdesc_spec(n_fft=400, hop_length=160)
        self.dim = dict(spectral_post=80, cond_spectral=80, trim_spectral=80, split_spectral=80, pitch=2, fdesc=6)
        self.sizes = {}  # out_rate -> (frames in front of the gate [S], intervals_stride)
        self.totals = {}  # (entry, out_rate) -> rows

    def submit(self):
        b = self.batch
        assert self.g.submit_host(b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"], flags=4)["rc"] == 0

    def bufs(self, name, q, n):
        chans, outs, _ = ENTRIES[name]
        T, ivs = self.sizes[q]
        shapes = dict(out=((n, chans or self.g.channels, int(T.max())), np.float32), frames=((n,), np.uint64), peaks=((n,), np.float32),
                      bounds=((n, 2), np.uint32), refs=((n,), np.float64), counts=((n,), np.uint32), iv=((n, ivs, 2), np.uint32),
                      rows=((self.totals.get((name, q), 0) + 1, self.dim.get(name, 40)), np.float32), seg_rows=((n,), np.uint64),
                      refused=((n,), np.uint32), status=((2,), np.uint32))
        return {k: np.full(shapes[k][0], K, shapes[k][1]) for k in outs}

    def call(self, name, q, b, S=None, fmt=2, stride=None, cap=None, ivs=None, null=None):
        """One raw call of the entry at out_rate q into the arrays of b: (rc, the message)."""
        from parseoggvorbis_amd.binding import Status
        S = self.S if S is None else S
        rates = np.full(S, RATE, np.uint32)
        p = types.SimpleNamespace(**{k: None if k == null else C.c_void_p(v.ctypes.data) for k, v in b.items()})
        st = C.cast(b["status"].ctypes.data, C.POINTER(Status)) if "status" in b else None
        stride = b["out"].shape[2] if stride is None and "out" in b else stride
        cap = b["rows"].shape[0] - 1 if cap is None and "rows" in b else cap
        ivs = b["iv"].shape[1] if ivs is None and "iv" in b else ivs
        L, h, r, err = self.lib, self.g.h, C.c_void_p(rates.ctypes.data), C.c_char_p()
        gate, cond, spec, post, e = C.byref(self.gate), C.byref(self.cond), C.byref(self.spec), C.byref(self.post), C.byref(err)
        if name == "resample":
            rc = L.vsyn_pcm_resample_host(h, S, r, q, fmt, p.out, stride, p.frames, e)
        elif name == "condition":
            rc = L.vsyn_pcm_condition_host(h, cond, S, r, q, fmt, p.out, stride, p.frames, p.peaks, e)
        elif name == "trim":
            rc = L.vsyn_pcm_trim_host(h, gate, cond, S, r, q, fmt, p.out, stride, p.frames, p.bounds, p.peaks, p.refs, e)
        elif name == "split":
            rc = L.vsyn_pcm_split_host(h, gate, cond, S, r, q, fmt, p.out, stride, p.frames, p.counts, p.iv, ivs, p.peaks, p.refs, e)
        elif name == "split_intervals":
            rc = L.vsyn_pcm_split_intervals_host(h, gate, S, r, q, p.frames, p.counts, p.iv, ivs, p.refs, e)
        elif name == "spectral":
            rc = L.vsyn_pcm_spectral_host(h, spec, S, r, p.rows, cap, p.seg_rows, st, e)
        elif name == "spectral_post":
            rc = L.vsyn_pcm_spectral_post_host(h, spec, post, S, r, q, p.rows, cap, p.seg_rows, st, e)
        elif name == "resample_spectral":
            rc = L.vsyn_pcm_resample_spectral_host(h, spec, S, r, q, p.rows, cap, p.seg_rows, st, e)
        elif name == "cond_spectral":
            rc = L.vsyn_pcm_cond_spectral_host(h, cond, spec, post, S, r, q, p.rows, cap, p.seg_rows, p.peaks, st, e)
        elif name == "trim_spectral":
            rc = L.vsyn_pcm_trim_spectral_host(h, gate, cond, spec, post, S, r, q, p.rows, cap, p.seg_rows, p.bounds, p.peaks, p.refs, st, e)
        elif name == "split_spectral":
            rc = L.vsyn_pcm_split_spectral_host(h, gate, cond, spec, post, S, r, q, p.rows, cap, p.seg_rows, p.frames, p.counts, p.iv, ivs,
                                                p.peaks, p.refs, st, e)
        elif name == "pitch":
            rc = L.vsyn_pcm_pitch_host(h, C.byref(self.pitch), S, r, q, p.rows, cap, p.seg_rows, p.refused, st, e)
        else:
            rc = L.vsyn_pcm_fdesc_host(h, C.byref(self.fdesc), S, r, q, p.rows, cap, p.seg_rows, p.refused, st, e)
        return rc, (err.value or b"").decode()

    def measure(self):
        """The sizes the accepted calls need, from the entries' own size queries."""
        for q in (0, OUT):
            self.sizes[q] = (np.ones(self.S, np.uint64), 1)
            b = self.bufs("condition", q, self.S)
            assert self.call("condition", q, b, null="out", stride=0) == (0, "")
            T = b["frames"].copy()
            self.sizes[q] = (T, int(self.lib.vsyn_pcm_split_max_intervals(C.byref(self.gate), int(T.max()))))
            assert T.min() > 0 and self.sizes[q][1] > 1
            for name, (_, outs, qs) in ENTRIES.items():
                if "rows" in outs and q in qs:
                    b = self.bufs(name, q, self.S)
                    assert self.call(name, q, b, null="rows", cap=0) == (0, ""), name
                    self.totals[name, q] = int(b["seg_rows"].sum())
                    assert self.totals[name, q] > 1, name

    def good(self, name, q):
        """The accepted call, every per-segment array one element longer than the call needs."""
        b = self.bufs(name, q, self.S + 1)
        assert self.call(name, q, b) == (0, ""), (name, q)
        for k, v in b.items():
            if k != "status":
                assert (v[self.S if k != "rows" else -1] == K).all(), (name, q, k)  # nothing behind the call's own
        return b


def _equal(a, b, k):
    """Output k of two calls, byte for byte; of the intervals, what the counts cover (the rest of a row is the workspace's)."""
    if k != "iv":
        return np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))
    return all(np.array_equal(p[:int(n)], q[:int(n)]) for p, q, n in zip(a["iv"], b["iv"], np.minimum(b["counts"], b["iv"].shape[1])))


def _same(a, b):
    return all(_equal(a, b, k) for k in a)


@pytest.fixture(scope="module")
def chain(mods):  # noqa: F811
    import torch
    assert torch.cuda.is_available()
    c, fresh = Chain(mods[1]), Chain(mods[1])
    c.submit()
    c.measure()
    fresh.sizes, fresh.totals = c.sizes, c.totals
    yield c, fresh
    c.g.close()
    fresh.g.close()


def _check_refused(c, name, q, fault, b, S_call, good, rc, msg):
    want = REFUSED[name][fault]
    assert rc == 1 and msg, (name, q, fault, rc, msg)
    S = c.S
    for k, v in b.items():
        state, w = want.get(k, KEPT), (name, q, fault, k)
        if state == KEPT:
            assert (v == K).all(), w
        elif state == RESET:
            assert v.tolist() == [0, 0xFFFFFFFF], w
        elif state == ZERO:
            assert not v[:S_call].any() and (v[S_call:] == K).all(), w
        elif state == UNGATED:
            assert np.array_equal(v[:S], c.sizes[q][0]) and (v[S:] == K).all(), w
        else:
            assert state == GOOD and _equal(b, good, k), w


def test_refusals_at_every_host_entry(chain):
    """REFUSED, fault by fault: VSYN_ERR_INVALID with a message, the outputs in the state the table gives, and the accepted call
    afterwards byte for byte what it was before. A handle without a submit refuses every entry; after its first submit it gives the
    other handle's bytes."""
    c, fresh = chain
    S, seen, goods = c.S, 0, {}
    for name, (_, outs, qs) in ENTRIES.items():
        for q in qs:
            good = goods[name, q] = c.good(name, q)
            if "frames" in outs and name in ("trim", "split", "split_spectral"):
                assert (good["frames"][:S] < c.sizes[q][0]).all(), (name, q)  # the gate cut every segment: UNGATED is not GOOD
            if "peaks" in outs:
                assert good["peaks"][:S].all(), (name, q)  # ZERO is not GOOD
            T, ivs = c.sizes[q]
            faults = dict(segments=dict(S=S + 1), null=dict(null="seg_rows" if "rows" in outs else "frames"))
            if "out" in outs:
                faults.update(format=dict(fmt=3), stride=dict(stride=int(T.max()) - 1))
            if "rows" in outs:
                faults["capacity"] = dict(cap=c.totals[name, q] - 1)
            if "iv" in outs:
                faults["ivs"] = dict(ivs=ivs - 1)
            assert set(faults) | {"no_submit"} == set(REFUSED[name]), name
            b = fresh.bufs(name, q, S + 1)
            _check_refused(fresh, name, q, "no_submit", b, S, good, *fresh.call(name, q, b))
            for fault, kw in faults.items():
                b = c.bufs(name, q, S + 1)
                _check_refused(c, name, q, fault, b, kw.get("S", S), good, *c.call(name, q, b, **kw))
                assert _same(c.good(name, q), good), (name, q, fault)
                seen += 1
    fresh.submit()
    for (name, q), good in goods.items():
        assert _same(fresh.good(name, q), good), (name, q)
    assert seen == 80  # 13 entries, 23 runs of them at a rate, the faults of each (the handle without a submit apart)


def test_nested_forms_agree_bit_for_bit(chain, mods):  # noqa: F811
    """A NULL gate, a NULL conditioning spec and a post stage that is off: the rows, row counts, PCM, frames and peaks of the entry
    without them, natively and resampled, float32 and int16. Then the chain entries, stage by stage (_chain_entries_nest; the
    loudness records of the fixture's short segments all carry status 2, VSYN_LOUD_TOO_SHORT)."""
    from parseoggvorbis_amd.binding import SpectralPost
    c, _ = chain
    g, s, S = c.g, c.spec, c.S
    off = SpectralPost(0, 3, 0, 0, 1e-5, None, None)
    rates = [RATE] * S
    for q in (0, OUT):
        base = g.pcm_spectral_post_host(s, off, rates, q)
        forms = [g.pcm_cond_spectral_host(None, s, None, rates, q), g.pcm_trim_spectral_host(None, None, s, None, rates, q),
                 g.pcm_split_spectral_host(None, None, s, None, rates, q)]
        if q == 0:
            forms.append(g.pcm_spectral_host(s, rates))
        raw = c.good("spectral" if q == 0 else "resample_spectral", q)
        assert base["rc"] == 0 and base["rows"].shape == (c.totals["spectral" if q == 0 else "resample_spectral", q], 40)
        assert np.array_equal(base["rows"].view(np.uint32), raw["rows"][:-1].view(np.uint32)) and np.array_equal(base["seg_rows"], raw["seg_rows"][:S])
        for i, f in enumerate(forms):
            assert f["rc"] == 0 and np.array_equal(f["seg_rows"], base["seg_rows"]), (q, i)
            assert np.array_equal(f["rows"].view(np.uint32), base["rows"].view(np.uint32)), (q, i)
        assert not forms[1]["bounds"].any() and not forms[1]["refs"].any() and not forms[2]["counts"].any() and not forms[2]["frames"].any()
        for cond in (_cond(), c.cond):
            for fmt in (2, 1):
                out, frames, peaks = g.pcm_condition_host(cond, S, rates, q, fmt)
                assert np.array_equal(frames, c.sizes[q][0])
                for f in (g.pcm_trim_host(None, cond, S, rates, q, fmt), g.pcm_split_host(None, cond, S, rates, q, fmt)):
                    assert f["pcm"].dtype == out.dtype and np.array_equal(f["pcm"].view(np.uint8), out.view(np.uint8)), (q, fmt)
                    assert np.array_equal(f["frames"], frames) and np.array_equal(f["peaks"].view(np.uint32), peaks.view(np.uint32)), (q, fmt)
                    assert not f["refs"].any()
    _chain_entries_nest(c, mods[1])


def _agree(wide, narrow, what):
    """The arrays two Synth methods returned (dicts, or pcm_condition_host's tuple), byte for byte: every one both have (of the
    intervals what the counts cover, which is what the methods return), and zeros in what the wider entry alone has."""
    if isinstance(narrow, tuple):
        narrow = dict(zip(("pcm", "frames", "peaks"), narrow))
    arrays = 0
    for k, v in wide.items():
        if k == "intervals":
            assert all(np.array_equal(p, q) for p, q in zip(v, narrow.get(k, [np.zeros((0, 2))] * len(v)))), (what, k)
        elif not isinstance(v, np.ndarray):
            assert k not in narrow or v == narrow[k], (what, k)
        elif k in narrow:
            assert v.dtype == narrow[k].dtype and np.array_equal(v.view(np.uint8), narrow[k].view(np.uint8)), (what, k)
            arrays += 1
        else:
            assert not v.view(np.uint8).any(), (what, k)
    assert not set(narrow) - set(wide) and arrays >= 2, what


def _chain_entries_nest(c, spectral):
    """The chain entries, each with its newest stage passed as NULL, against the entry without that stage, down to the gated
    entries: out_rate 0 and OUT, no gate, a trim and a split, float32 and int16 for the PCM forms, the stages that stay on in both
    calls of a pair at the smallest specs they accept. The fixture's segments are a fraction of a second: the normaliser reports
    every one VSYN_LOUD_TOO_SHORT (record status 2), so the pairs bind the plumbing and not the stage."""
    from parseoggvorbis_amd.binding import LoudnessSpec, PcmEffect, SpectralHpss, VSYN_LOUD_MONO, VSYN_LOUD_NORMALIZE, VSYN_LOUD_TOO_SHORT
    g, S = c.g, c.S
    rates = [RATE] * S
    loud = LoudnessSpec(VSYN_LOUD_NORMALIZE, VSYN_LOUD_MONO, -23.0)
    hpss = SpectralHpss(5, 5, 0, 0, 2.0, 1.0, 1.0)
    effect = PcmEffect(256, 64, 256, 0, hpss)
    pre = _cond(False, A)  # (the normaliser excludes the peak)
    power = spectral.spectral_spec(kind="mel_power", n_fft=400, hop_length=160, n_mels=40)  # (what HPSS and PCEN take)
    pcen = spectral.pcen_spec()
    for q in (0, OUT):
        for name, gate, split in (("none", None, 0), ("trim", c.gate, 0), ("split", c.gate, 1)):
            for fmt in (2, 1):
                w = (q, name, fmt)
                eff = g.pcm_chain_effects_host(gate, split, effect, loud, pre, S, rates, q, fmt)
                assert (eff["records"]["status"] == VSYN_LOUD_TOO_SHORT).all(), (w, eff["records"]["status"])
                _agree(g.pcm_chain_stretch_host(gate, split, effect, None, None, None, loud, pre, S, rates, q, fmt), eff, (w, "stretch"))
                _agree(g.pcm_chain_effects_host(gate, split, None, loud, pre, S, rates, q, fmt),
                       g.pcm_chain_host(gate, split, loud, pre, S, rates, q, fmt), (w, "effect"))
                gated = (g.pcm_condition_host(c.cond, S, rates, q, fmt) if gate is None else
                         g.pcm_split_host(gate, c.cond, S, rates, q, fmt) if split else g.pcm_trim_host(gate, c.cond, S, rates, q, fmt))
                _agree(g.pcm_chain_host(gate, split, None, c.cond, S, rates, q, fmt), gated, (w, "loud"))
            w = (q, name)
            _agree(g.pcm_chain_rhythm_host(gate, split, loud, pre, power, None, hpss, pcen, None, None, rates, q),
                   g.pcm_chain_hpss_host(gate, split, loud, pre, power, None, hpss, pcen, None, rates, q), (w, "rhythm"))
            _agree(g.pcm_chain_hpss_host(gate, split, loud, pre, power, None, None, pcen, None, rates, q),
                   g.pcm_chain_chroma_host(gate, split, loud, pre, power, None, pcen, None, rates, q), (w, "hpss"))
            _agree(g.pcm_chain_chroma_host(gate, split, loud, pre, c.spec, None, None, c.post, rates, q),
                   g.pcm_chain_spectral_host(gate, split, loud, pre, c.spec, None, c.post, rates, q), (w, "chroma"))
            pcen_form = g.pcm_split_spectral_pcen_host if split else g.pcm_trim_spectral_pcen_host
            _agree(g.pcm_chain_spectral_host(gate, split, None, c.cond, power, pcen, None, rates, q),
                   pcen_form(gate, c.cond, power, pcen, None, rates, q), (w, "loud, rows"))
            _agree(pcen_form(gate, c.cond, c.spec, None, c.post, rates, q),
                   (g.pcm_split_spectral_host if split else g.pcm_trim_spectral_host)(gate, c.cond, c.spec, c.post, rates, q), (w, "pcen"))


# the middle segment at eight times the others' rate: resampled to OUT it is a sixteenth of its frames long
SHORT_RATES = [RATE, 8 * RATE, RATE]
SHORT_ROWS = {"ungated": [13, 2, 16], "trim": [13, 2, 16], "split": [13, 2, 16]}  # (a 60 dB gate cuts nothing off these)


def test_a_segment_below_the_delta_width(chain):
    """Delta width 5 and a segment of fewer rows: behind a gate that segment alone has no rows and the others have theirs; without
    a gate the call is refused."""
    from parseoggvorbis_amd.binding import SpectralPost, VsynError
    c, _ = chain
    g, s = c.g, c.spec
    post = SpectralPost(1, 5, 0, 0, 1e-5, None, None)
    wide = _trim(60.0, 400, 160)
    plain = g.pcm_cond_spectral_host(None, s, None, SHORT_RATES, OUT)
    print("rows per segment, ungated:", plain["seg_rows"].tolist())
    assert plain["seg_rows"].tolist() == SHORT_ROWS["ungated"]
    assert 0 < plain["seg_rows"][1] < 5 <= min(plain["seg_rows"][0], plain["seg_rows"][2])
    with pytest.raises(VsynError, match="segment 1: delta width 5 needs 5 frames") as ei:
        g.pcm_cond_spectral_host(None, s, post, SHORT_RATES, OUT)
    assert ei.value.code == 1
    for name, form in (("trim", g.pcm_trim_spectral_host), ("split", g.pcm_split_spectral_host)):
        bare = form(wide, None, s, None, SHORT_RATES, OUT)
        got = form(wide, None, s, post, SHORT_RATES, OUT)
        print("rows per segment, %s:" % name, bare["seg_rows"].tolist(), got["seg_rows"].tolist())
        assert bare["seg_rows"].tolist() == SHORT_ROWS[name]
        assert 0 < bare["seg_rows"][1] < 5 and got["rc"] == 0
        assert got["seg_rows"].tolist() == [bare["seg_rows"][0], 0, bare["seg_rows"][2]]
        assert got["rows"].shape == (int(got["seg_rows"].sum()), 80) and np.isfinite(got["rows"]).all()
        n0 = int(bare["seg_rows"][0])
        assert np.array_equal(got["rows"][:n0, :40].view(np.uint32), bare["rows"][:n0].view(np.uint32))
        assert np.array_equal(got["rows"][n0:, :40].view(np.uint32), bare["rows"][n0 + int(bare["seg_rows"][1]):].view(np.uint32))
        assert np.isfinite(got["refs"]).all()
