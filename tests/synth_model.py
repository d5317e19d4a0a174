"""Float64 model of the synthesis after the envelope, and the per-packet gate the synthesis PCM is held to. numpy only.

Input: the "after_envelope" tensor (inverse coupling + floor product, hpp:1213-1255), a float32 quantity the reference defines and
the device reproduces bit for bit; the model takes it from the CPU oracle's tap. Everything after it is done in float64 from the
stated semantics:
  IMDCT         y_i = sum_k X_k cos(2pi/n (i + 1/2 + n/4)(k + 1/2)), i < n, k < n/2 (orc_imdct_closed_form), through numpy.fft
  windows       the Vorbis power-sine slopes, sin(pi/2 sin^2(pi/2 (i + 1/2) / len)), placed as orc_window places them: the left
                slope follows prev_long, the right one next_long; short blocks ignore both flags
  overlap-add   the reference's decode state (hpp:975-1115; the oracle's state_begin_packet / state_advance / state_add_frame /
                state_forward) with its sliding buffer, granule trimming, VSYN_SEG_RESET and streams continuing across submits
Per packet p and channel c the model also returns the scale s[p, c] = max(rms(y_{p-1}), rms(y_p)) of the unwindowed IMDCT outputs
whose windowed halves make up p's emitted frames. The gate is

    max over p's emitted frames of |got - model| <= G * 2^-24 * s[p, c], and got == 0 exactly where s[p, c] == 0.

G = 96. Measured (max |got - model| / (2^-24 s), worst packet): the oracle, i.e. the reference's own float32 arithmetic, 24 on the
parity suite's synthetic shapes, 22 on the loudness profiles, 25 on the reference's fixtures (its own pcm hook: 25 / 17), and 77 on
the synth_NN fixtures (synth_12, packet 7: a long block whose peak is 13 times its rms, so that errors relative to the local value
are large against the block's rms); the device 17 on the tuned 256/2048 kernel (ring mode 14), 16 on the size-generic kernel,
18 on the staged kernels, 16 on the IMDCT-only entry. One gate for the oracle and the device: as accurate as the reference.
Scope: window flags that agree with the block sequence (flags that disagree keep their exact oracle tests)."""
import hashlib

import numpy as np

G = 96.0
ULP = 2.0 ** -24


def imdct(n, x):
    """x [rows][n/2] -> float64 [rows][n]: y_i = sum_k x_k cos(2pi/n (i + 1/2 + n/4)(k + 1/2)), O(n log n) per row.
    With n0 = 1/2 + n/4: y_i = Re(e^{i pi (i + n0)/n} sum_k (x_k e^{2 pi i n0 k/n}) e^{2 pi i i k/n})."""
    x = np.asarray(x, np.float64).reshape(-1, n // 2)
    n0 = 0.5 + n / 4.0
    k = np.arange(n // 2)
    z = np.zeros((x.shape[0], n), np.complex128)
    z[:, :n // 2] = x * np.exp(2j * np.pi * n0 * k / n)
    i = np.arange(n)
    return (np.fft.ifft(z, axis=1) * n * np.exp(1j * np.pi * (i + n0) / n)).real


def window(bs0, bs1, long_block, prev, nxt):
    """Float64 Vorbis window of one block (orc_window's placement; short blocks ignore prev / nxt)."""
    n = bs1 if long_block else bs0
    if not long_block:
        prev = nxt = False
    left, right = (bs1 if prev else bs0) // 2, (bs1 if nxt else bs0) // 2
    lb, rb = n // 4 - left // 2, n - n // 4 - right // 2
    w = np.zeros(n)

    def slope(m):
        x = np.sin(np.pi / 2 * (np.arange(m) + 0.5) / m)
        return np.sin(np.pi / 2 * x * x)

    w[lb:lb + left] = slope(left)
    w[lb + left:rb] = 1.0
    w[rb:rb + right] = slope(right)[::-1]
    return w


def agreeing_flags(spec, packets, segments):
    """True if every long packet's prev_long / next_long agree with the blocks around it in its segment (the model's scope; the
    first packet of a segment that continues a stream and the last packet of every segment are free)."""
    lng = np.array([spec.modes[int(m)][0] for m in packets["mode"]], bool)
    for sg in segments:
        a, k = int(sg["first_packet"]), int(sg["num_packets"])
        for q in range(k):
            p = a + q
            if not lng[p]:
                continue
            if q > 0 and bool(packets["prev_long"][p]) != lng[p - 1]:
                return False
            if q + 1 < k and bool(packets["next_long"][p]) != lng[p + 1]:
                return False
    return True


class _State:
    """The reference's VorbisStreamDecodeState (hpp:975-1115) in float64, plus the rms of the last block per channel."""

    def __init__(self, channels, cap):
        self.buf = np.zeros((channels, cap))
        self.cap = cap
        self.reset()

    def reset(self):
        self.buf[:] = 0
        self.pcm_offset = 0
        self.pshwo = 0  # prev_second_half_window_off
        self.prev_win = self.cur_win = 0
        self.abs_total_pos = 0
        self.expected_end = 0
        self.last_rms = np.zeros(self.buf.shape[0])

    def advance(self, next_win):  # hpp:1069-1109
        cur = self.cur_win
        second_half = self.pcm_offset + cur // 2
        next_off = self.pcm_offset + (cur // 4) * 3 - next_win // 4
        if next_off + next_win >= self.cap:  # slide left, keep the second half
            needed = self.pcm_offset + cur // 2 - next_off
            second_half = max(needed, 0)
            src = self.buf[:, self.pcm_offset + cur // 2: self.pcm_offset + cur].copy()
            self.buf[:, second_half:second_half + cur // 2] = src
            self.buf[:, second_half + cur // 2:] = 0
            next_off = -needed if needed < 0 else 0
        elif next_off < 0:  # short then long: slide right
            extra = -next_off
            second_half += extra
            src = self.buf[:, self.pcm_offset:self.pcm_offset + cur].copy()
            self.buf[:, self.pcm_offset + extra:self.pcm_offset + extra + cur] = src
            self.buf[:, :self.pcm_offset + extra] = 0
            next_off = 0
        if next_win < cur and not next_off > 0:
            raise ValueError("decode state: next block does not fit (hpp:1104-1105)")
        self.pshwo = second_half - next_off
        self.pcm_offset = next_off

    def begin_packet(self, win):  # hpp:1061-1067
        if self.cur_win > 0:
            self.advance(win)
        self.prev_win, self.cur_win = self.cur_win, win

    def forward(self):  # hpp:1019-1059 -> frames [channels][k], or None where the reference fails a CHECK
        frames = self.prev_win // 4 + self.cur_win // 4 if self.prev_win > 0 else 0
        if self.expected_end >= 0:
            if self.abs_total_pos > self.expected_end or self.abs_total_pos + frames < self.expected_end:
                return None
            frames = self.expected_end - self.abs_total_pos
        a = self.pcm_offset + self.pshwo
        out = self.buf[:, a:a + frames].copy()
        self.abs_total_pos += frames
        return out


class SynthModel:
    """Float64 model with the submit surface of OracleSynth / Synth.submit_host. submit_host(..., envelope=None) takes the
    after_envelope tensor from the CPU oracle (a handle of its own, fed the same submits, so that streams continue alike) unless
    it is given. Returns dict(rc, pcm float64 [S][C][plane_stride], emit_len [P], scale [P][C], n [P])."""

    def __init__(self, spec, max_streams=64):
        self.spec = spec
        self.channels = spec.channels
        self.cap = 5 * spec.blocksize0 + 5 * spec.blocksize1  # hpp:1359
        self.st = [None] * max_streams
        self._oracle = None
        self._win = {}

    def reset(self):
        self.st = [None] * len(self.st)
        if self._oracle is not None:
            self._oracle.reset()

    def _window(self, lng, prev, nxt):
        key = (lng, prev, nxt) if lng else (0, 0, 0)
        if key not in self._win:
            self._win[key] = window(self.spec.blocksize0, self.spec.blocksize1, *key)
        return self._win[key]

    def submit_host(self, packets, segments, ys, residue, plane_stride, envelope=None):
        from tests.workloads import packet_blocks
        spec, Cn = self.spec, self.channels
        if envelope is None:
            if self._oracle is None:
                from oracle.oracle_binding import OracleSynth
                self._oracle = OracleSynth(spec, len(self.st))
            o = self._oracle.submit_host(packets, segments, ys, residue, plane_stride, want_taps=True)
            assert o["rc"] == 0, (o["rc"], o["flags"], o["first_bad"])
            envelope = o["taps"]["after_envelope"]
        assert agreeing_flags(spec, packets, segments), "the model covers window flags that agree with the block sequence only"
        envelope = np.asarray(envelope, np.float32)
        P, S = len(packets), len(segments)
        n_of, off = packet_blocks(spec, packets, segments)
        # every block's float64 IMDCT, batched per block size
        y = [None] * P
        in_seg = np.zeros(P, bool)
        for sg in segments:
            in_seg[int(sg["first_packet"]):int(sg["first_packet"]) + int(sg["num_packets"])] = True
        for n in np.unique(n_of[in_seg]):
            ps = np.flatnonzero(in_seg & (n_of == n))
            idx = (off[ps][:, None] + np.arange(Cn * n // 2)[None, :])
            blocks = imdct(int(n), envelope[idx].reshape(-1, n // 2)).reshape(len(ps), Cn, n)
            for j, p in enumerate(ps):
                y[p] = blocks[j]
        pcm = np.zeros((S, Cn, plane_stride))
        emit = np.zeros(P, np.uint32)
        scale = np.zeros((P, Cn))
        for g, sg in enumerate(segments):
            s = int(sg["stream"])
            if self.st[s] is None:
                self.st[s] = _State(Cn, self.cap)
            st = self.st[s]
            if int(sg["flags"]) & 1:  # VSYN_SEG_RESET
                st.reset()
            written = 0
            for p in range(int(sg["first_packet"]), int(sg["first_packet"]) + int(sg["num_packets"])):
                n = int(n_of[p])
                lng = bool(spec.modes[int(packets["mode"][p])][0])
                st.begin_packet(n)
                st.buf[:, st.pcm_offset:st.pcm_offset + n] += y[p] * self._window(lng, bool(packets["prev_long"][p]),
                                                                                  bool(packets["next_long"][p]))
                rms = np.sqrt(np.mean(y[p] * y[p], axis=1))
                scale[p] = np.maximum(st.last_rms, rms)
                st.last_rms = rms
                st.expected_end = int(packets["granule"][p])
                out = st.forward()
                if out is None:
                    raise ValueError("granule check fails at packet %d" % p)
                k = out.shape[1]
                assert written + k <= plane_stride
                pcm[g, :, written:written + k] = out
                emit[p] = k
                written += k
        return dict(rc=0, pcm=pcm, emit_len=emit, scale=scale, n=n_of)


def per_packet_error(got_pcm, model, segments, emit_len=None):
    """-> ratio [P][C]: max over packet p's emitted frames of |got - model| / (2^-24 s[p, c]); inf where s == 0 and got != 0,
    0 where both are 0. emit_len: the frame counts of `got` (must equal the model's)."""
    emit = model["emit_len"] if emit_len is None else emit_len
    assert np.array_equal(np.asarray(emit), model["emit_len"])
    P, Cn = model["scale"].shape
    ratio = np.zeros((P, Cn))
    for g, sg in enumerate(segments):
        a, k = int(sg["first_packet"]), int(sg["num_packets"])
        e = model["emit_len"][a:a + k].astype(np.int64)
        tot = int(e.sum())
        if not tot:
            continue
        d = np.abs(np.asarray(got_pcm[g][:, :tot], np.float64) - model["pcm"][g][:, :tot])  # [C][tot]
        starts = np.concatenate([[0], np.cumsum(e)[:-1]])
        has = e > 0
        worst = np.maximum.reduceat(d, starts[has], axis=1).T  # [packets with frames][C]
        s = model["scale"][a:a + k][has]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(s > 0, worst / (ULP * np.where(s > 0, s, 1.0)), np.where(worst > 0, np.inf, 0.0))
        ratio[a:a + k][has] = r
    return ratio


def gate(got_pcm, model, segments, emit_len=None, g=G, ctx=None):
    """Assert the per-packet gate; returns the worst ratio (in units of 2^-24 s)."""
    r = per_packet_error(got_pcm, model, segments, emit_len)
    worst = float(r.max()) if r.size else 0.0
    if not worst <= g:
        p, c = np.unravel_index(int(np.argmax(r)), r.shape)
        raise AssertionError("per-packet gate: packet %d channel %d at %.3g x 2^-24 s (gate %g), n %d, s %.3g %s"
                             % (p, c, r[p, c], g, model["n"][p], model["scale"][p, c], ctx or ""))
    return worst


def worst_by_block_size(ratio, n):
    """{block size: worst ratio} of per_packet_error's result."""
    return {int(k): float(ratio[n == k].max()) for k in np.unique(n) if ratio[n == k].size}


_CACHE = {}


def _key(spec, b):
    h = hashlib.sha1()
    h.update(repr((spec.channels, spec.blocksize0, spec.blocksize1, spec.floors, spec.mappings, spec.modes)).encode())
    for k in ("packets", "segments", "ys", "residue"):
        h.update(np.ascontiguousarray(b[k]).tobytes())
    h.update(str(int(b["plane_stride"])).encode())
    return h.hexdigest()


def model_of(spec, b):
    """The model of batch b (every stream starting fresh), computed once per batch and kept for the other paths of a test."""
    k = _key(spec, b)
    if k not in _CACHE:
        if len(_CACHE) > 8:
            _CACHE.clear()
        _CACHE[k] = SynthModel(spec, max(1, int(b["segments"]["stream"].max()) + 1) if len(b["segments"]) else 1).submit_host(
            b["packets"], b["segments"], b["ys"], b["residue"], b["plane_stride"])
    return _CACHE[k]


def check_model(got, spec, b, ctx=None):
    """The per-packet gate of got (a submit_host result) against the model of batch b (cached)."""
    return gate(got["pcm"], model_of(spec, b), b["segments"], got["emit_len"], ctx=ctx)
