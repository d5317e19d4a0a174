"""Shared inputs for tests and bench: the committed golden fixtures and the seeded synthetic batches of
BASELINE.json's configs.  numpy only."""
import os

import numpy as np

from parseoggvorbis_amd.binding import PACKET_DTYPE, SEGMENT_DTYPE, VSYN_SEG_RESET, SetupSpec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# floor-1 X lists of the reference's fixtures (hook "floor1_unpack xs", hpp:1367)
FIX_XS_SHORT = [0, 128, 14, 4, 58, 2, 8, 28, 90]
FIX_XS_LONG_SORTED = [0, 3, 6, 10, 14, 18, 23, 28, 33, 39, 46, 55, 65, 79, 93, 111, 130, 158, 186, 220, 260, 312, 372,
                      464, 556, 650, 750, 850, 1024]


def load_golden(name):
    """-> (SetupSpec, dict of arrays, npz) for 'test.stereo44khz' / 'test.mono44khz'."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    C = int(z["channels"])
    floors = [(int(z["floor%d_mult" % f]), [int(v) for v in z["floor%d_xs" % f]]) for f in range(int(z["num_floors"]))]
    coup = [(0, 1)] if C == 2 else []
    # fixtures: mode 0 short -> mapping 0 -> floor 0, mode 1 long -> mapping 1 -> floor 1
    spec = SetupSpec(C, int(z["blocksize0"]), int(z["blocksize1"]), floors,
                     [(coup, [0] * C), (coup, [1] * C)], [(0, 0), (1, 1)])
    P = len(z["mode"])
    assert np.array_equal(z["floor_number"], np.repeat(z["mode"][:, None], C, 1))
    pk = np.zeros(P, PACKET_DTYPE)
    pk["mode"], pk["prev_long"], pk["next_long"] = z["mode"], z["prev_long"], z["next_long"]
    pk["floor_used"], pk["granule"] = z["floor_used"], z["granule"]
    seg = np.zeros(1, SEGMENT_DTYPE)
    seg["num_packets"], seg["flags"] = P, VSYN_SEG_RESET
    return spec, dict(packets=pk, segments=seg, ys=z["ys"], residue=z["residue"], pcm=z["pcm"],
                      emit_len=z["emit_len"]), z


def fixture_like_spec(channels=2, bs0=256, bs1=2048, coupled=True):
    """The fixtures' stream setup, generalised to other blocksizes by scaling the X lists (coupled=False: no coupling step)."""
    def scale(xs, n2, base):
        out = sorted({min(n2, max(0, (x * n2) // base)) for x in xs})
        if len(out) < 2:
            out = [0, n2]
        out = [0, n2] + [x for x in out if x not in (0, n2)]
        return out
    short = scale(FIX_XS_SHORT, bs0 // 2, 128)
    long_sorted = scale(FIX_XS_LONG_SORTED, bs1 // 2, 1024)
    rng = np.random.default_rng(99)
    inner = long_sorted[2:]
    rng.shuffle(inner)  # header order is not sorted in real streams
    long_ = [0, bs1 // 2] + [int(v) for v in inner]
    coup = [(0, 1)] if channels >= 2 and coupled else []
    return SetupSpec(channels, bs0, bs1, [(4, short), (2, long_)],
                     [(coup, [0] * channels), (coup, [1] * channels)], [(0, 0), (1, 1)])


def _encode_ys(xs, mult, target, rng, zero_frac):
    """Coded floor-1 ys whose unwrap gives (approximately) `target` amplitudes; always in range (valid stream)."""
    rng_of = {1: 256, 2: 128, 3: 86, 4: 64}[mult]
    posts = len(xs)
    ys = np.zeros(posts, np.int64)
    fy = np.zeros(posts, np.int64)
    lo_n = [max([j for j in range(i) if xs[j] < xs[i]], key=lambda j: xs[j], default=-1) for i in range(posts)]
    hi_n = [min([j for j in range(i) if xs[j] > xs[i]], key=lambda j: xs[j], default=-1) for i in range(posts)]
    fy[0] = ys[0] = min(rng_of - 1, max(0, int(target[0])))
    fy[1] = ys[1] = min(rng_of - 1, max(0, int(target[1])))
    for i in range(2, posts):
        lo, hi = lo_n[i], hi_n[i]
        adx = xs[hi] - xs[lo]
        dy = fy[hi] - fy[lo]
        off = (abs(dy) * (xs[i] - xs[lo])) // adx
        pred = fy[lo] + off if dy >= 0 else fy[lo] - off
        d = min(rng_of - 1, max(0, int(target[i]))) - pred
        hr, lr = rng_of - pred, pred
        room = min(hr, lr) * 2
        val = 0
        if d != 0 and rng.random() >= zero_frac:
            if d > 0:
                val = 2 * d if 2 * d < room else (d + lr if hr > lr else 0)
            else:
                val = -2 * d - 1 if -2 * d - 1 < room else (hr - d - 1 if hr <= lr else 0)
        if val == 0:
            f = pred
        elif val >= room:
            f = val - lr + pred if hr > lr else pred - val + hr - 1
        else:
            f = pred - (val + 1) // 2 if val % 2 else pred + val // 2
        if not (0 <= f < rng_of):
            val, f = 0, pred
        ys[i], fy[i] = val, f
    return ys


QUIET_YS = (0, 8)      # floor range of quiet packets: peak |pcm| about 5e-5 with the default residue
LOUD_YS = (150, 250)   # floor range of loud packets: peak |pcm| about 150


def synth_batch(spec, streams, packets_per_stream, pattern="long", seed=1234, ylo=28, yhi=88, unused_frac=0.0,
                granule_last=False, roll=True, prev_long=None, next_long=None, residue="laplace", residue_scale=1.0,
                floor_ranges=None, alternate=0, modes=None):
    """Synthetic batch in the shape of BASELINE configs 3/4:
    residue = round(Laplace(b=1.5)) with 60 % zeros; floor amplitudes a random walk in [ylo,yhi] (step +-6)
    over the setup's X list, wrapped into coded ys.  pattern: 'long', 'short', 'mixed' (L L L S*8 repeating, rotated per
    stream) or an explicit sequence of block flags (1 = long), the same for every stream.
    prev_long / next_long: window flag bytes of every packet of the batch ([streams * packets_per_stream], short packets included),
    instead of the flags that agree with the block sequence (disagreeing_window_flags); the batch is otherwise the same.
    Precision probes (the defaults leave the batch unchanged, byte for byte):
    residue: 'laplace' (the above) or 'gauss' (standard normal: dense, non-integer, no zeros, more cancellation in the IMDCT),
    times residue_scale; floor_ranges: one (ylo, yhi) per stream instead of (ylo, yhi); alternate=k: packets alternate between
    k quiet packets (floor range QUIET_YS) and k loud ones (LOUD_YS) within each segment, loud first, so that overlap carries run
    from loud blocks into quiet ones.
    modes: the mode number of every packet, [streams * packets_per_stream] or a callable (stream, q) -> mode, instead of the setup's
    first long and first short mode laid out by `pattern` (which is then ignored): the block flag, the window flags, the residue
    length and the floor of each channel follow from the packet's mode (None leaves the batch unchanged, byte for byte).
    Returns dict(packets, segments, ys, residue, plane_stride)."""
    assert residue in ("laplace", "gauss"), residue
    rng = np.random.default_rng(seed)
    C = spec.channels
    if not isinstance(pattern, str):
        flags1 = np.asarray(pattern, np.uint8)
        assert len(flags1) == packets_per_stream
        roll = False
    elif pattern == "long":
        flags1 = np.ones(packets_per_stream, np.uint8)
    elif pattern == "short":
        flags1 = np.zeros(packets_per_stream, np.uint8)
    else:
        unit = [1, 1, 1] + [0] * 8
        flags1 = np.array((unit * (packets_per_stream // len(unit) + 1))[:packets_per_stream], np.uint8)
    P = streams * packets_per_stream
    if modes is None:
        long_mode = [i for i, (bf, _) in enumerate(spec.modes) if bf][0]
        short_mode = [i for i, (bf, _) in enumerate(spec.modes) if not bf][0]
        stream_flags = [flags1 if (not roll or pattern != "mixed") else np.roll(flags1, s % 11) for s in range(streams)]
        stream_modes = [np.where(f, long_mode, short_mode) for f in stream_flags]
    else:
        if callable(modes):
            modes = [modes(s, q) for s in range(streams) for q in range(packets_per_stream)]
        stream_modes = np.asarray(modes, np.int64).reshape(streams, packets_per_stream)
        assert 0 <= stream_modes.min() and stream_modes.max() < len(spec.modes)
        stream_flags = [np.array([1 if spec.modes[int(m)][0] else 0 for m in row], np.uint8) for row in stream_modes]
    pk = np.zeros(P, PACKET_DTYPE)
    seg = np.zeros(streams, SEGMENT_DTYPE)
    stride = spec.ys_stride
    ys = np.zeros((P, C, stride), np.uint16)
    res_parts = []
    off = 0
    for s in range(streams):
        flags = stream_flags[s]
        seg[s] = (s, s * packets_per_stream, packets_per_stream, VSYN_SEG_RESET, off)
        for q in range(packets_per_stream):
            p = s * packets_per_stream + q
            lng = int(flags[q])
            mode = int(stream_modes[s][q])
            n = spec.blocksize1 if lng else spec.blocksize0
            pk[p]["mode"] = mode
            if lng:
                pk[p]["prev_long"] = flags[q - 1] if q > 0 else 1
                pk[p]["next_long"] = flags[q + 1] if q + 1 < packets_per_stream else 1
            pk[p]["granule"] = -1
            lo, hi = (ylo, yhi) if floor_ranges is None else floor_ranges[s]
            if alternate:
                lo, hi = QUIET_YS if (q // alternate) % 2 else LOUD_YS
            used = 0
            for c in range(C):
                if rng.random() < unused_frac:
                    continue
                used |= 1 << c
                mult, xs = spec.floors[spec.mappings[spec.modes[mode][1]][1][c]]
                order = np.argsort(xs)
                walk = np.clip(np.cumsum(rng.integers(-6, 7, len(xs))) + rng.integers(lo, hi), lo, hi)
                target = np.zeros(len(xs), np.int64)
                target[order] = walk * 2 // mult  # same dB range whatever the multiplier
                ys[p, c, :len(xs)] = _encode_ys(xs, mult, target, rng, 0.25)
            pk[p]["floor_used"] = used
            if residue == "laplace":
                r = np.round(rng.laplace(0.0, 1.5, (C, n // 2)))
                r[rng.random((C, n // 2)) < 0.6] = 0
            else:
                r = rng.standard_normal((C, n // 2))
            if residue_scale != 1.0:
                r = r * residue_scale
            res_parts.append(r.astype(np.float32).ravel())
            off += C * (n // 2)
    if prev_long is not None:
        pk["prev_long"] = np.asarray(prev_long, np.uint8)
    if next_long is not None:
        pk["next_long"] = np.asarray(next_long, np.uint8)
    if granule_last:
        for s in range(streams):
            sizes = np.where(stream_flags[s], spec.blocksize1, spec.blocksize0)
            total = int(sum(sizes[i - 1] // 4 + sizes[i] // 4 for i in range(1, packets_per_stream)))
            last_l = int(sizes[-2] // 4 + sizes[-1] // 4) if packets_per_stream > 1 else 0
            pk[s * packets_per_stream + packets_per_stream - 1]["granule"] = total - min(37, last_l // 2)  # clipped last packet
    plane = packets_per_stream * (spec.blocksize1 // 2) + 64
    return dict(packets=pk, segments=seg, ys=ys, residue=np.concatenate(res_parts), plane_stride=plane)


def concat_batches(parts):
    """One batch from several synth_batch results (segments renumbered onto consecutive streams)."""
    pk = np.concatenate([p["packets"] for p in parts])
    ys = np.concatenate([p["ys"] for p in parts])
    res = np.concatenate([p["residue"] for p in parts])
    segs = np.concatenate([p["segments"] for p in parts]).copy()
    first = res_off = 0
    i = 0
    for p in parts:
        for s in range(len(p["segments"])):
            segs[i]["stream"] = i
            segs[i]["first_packet"] = first + p["segments"][s]["first_packet"]
            segs[i]["residue_off"] = res_off + p["segments"][s]["residue_off"]
            i += 1
        first += len(p["packets"])
        res_off += len(p["residue"])
    return dict(packets=pk, segments=segs, ys=ys, residue=res, plane_stride=max(p["plane_stride"] for p in parts))


def packet_blocks(spec, packets, segments):
    """-> (n [P], residue offset [P]) of a batch: every packet's block size and the float index of its first residue value."""
    n = np.array([spec.blocksize1 if spec.modes[int(m)][0] else spec.blocksize0 for m in packets["mode"]], np.int64)
    off = np.zeros(len(packets), np.int64)
    for sg in segments:
        a, k = int(sg["first_packet"]), int(sg["num_packets"])
        sizes = n[a:a + k] // 2 * spec.channels
        off[a:a + k] = int(sg["residue_off"]) + np.concatenate([[0], np.cumsum(sizes)[:-1]]) if k else []
    return n, off


def silence(spec, b, packets, channels=None):
    """Make channels (default: all) of the given packets silent in place, as a real decoder delivers an unused channel: floor_used
    cleared and the residue zeroed."""
    n, off = packet_blocks(spec, b["packets"], b["segments"])
    chans = range(spec.channels) if channels is None else channels
    for p in packets:
        for c in chans:
            b["packets"][p]["floor_used"] &= ~np.uint32(1 << c)
            b["residue"][off[p] + c * n[p] // 2: off[p] + (c + 1) * n[p] // 2] = 0
    return b


def loudness_profiles(spec, npk=24, seed=1):
    """The loudness profiles of the precision tests, one batch each for spec's block sizes: quiet (peak about 5e-5), loud (about
    1e5), a quiet and a loud stream in one submit, alternating loud and quiet packets, Gaussian residue, silent channels."""
    pat = "long" if spec.blocksize0 == spec.blocksize1 else "mixed"
    quiet = synth_batch(spec, 2, npk, pat, seed=seed, ylo=0, yhi=8, granule_last=True)  # no unused channel: its residue is loud
    loud = synth_batch(spec, 2, npk, pat, seed=seed + 1, ylo=150, yhi=250, residue_scale=1000.0, granule_last=True)
    both = synth_batch(spec, 2, npk, pat, seed=seed + 2, floor_ranges=[(0, 8), (150, 250)], granule_last=True)
    alt = concat_batches([synth_batch(spec, 1, npk, pat, seed=seed + 3, alternate=1),
                          synth_batch(spec, 1, npk, "long", seed=seed + 4, alternate=3, granule_last=True)])
    gauss = synth_batch(spec, 2, npk, pat, seed=seed + 5, residue="gauss", granule_last=True)
    sil = synth_batch(spec, 3, npk, pat, seed=seed + 6, alternate=2)
    silence(spec, sil, [q for q in range(npk) if q % 5 in (1, 2)])              # every channel, after and before loud packets
    if not any(m[0] for m in spec.mappings):  # one whole channel of stream 1 (a coupled partner would bring it back to life)
        silence(spec, sil, range(npk, 2 * npk), channels=[spec.channels - 1])
    silence(spec, sil, range(2 * npk, 3 * npk))                                 # a whole stream
    return dict(quiet=quiet, loud=loud, both=both, alternate=alt, gauss=gauss, silent=sil)


FLAG_BYTES = np.array([0, 1, 2, 0x80, 255], np.uint8)  # the reference treats any non-zero byte as true (getWindow(bool, bool))


def disagreeing_window_flags(rng, blocks, bs0, bs1, allow_a=False):
    """Window flag bytes drawn at random (0, 1, 2, 0x80, 255) for every packet of one stream, whatever the blocks around it.
    blocks: block flags of the stream (1 = long). Each of classes B, C and D (window_flag_classes) is forced at least once where the
    blocks allow it. Unless allow_a, a long block followed by a smaller one gets next_long = 0: that case (class A,
    VSYN_ST_WINDOW_FLAGS) is refused by the device; the three others stay exact. -> (prev_long, next_long)"""
    blocks = np.asarray(blocks, np.uint8)
    n = len(blocks)
    prev = FLAG_BYTES[rng.integers(0, len(FLAG_BYTES), n)]
    nxt = FLAG_BYTES[rng.integers(0, len(FLAG_BYTES), n)]
    lg = blocks == 1
    at_b = np.flatnonzero(~lg[:-1] & lg[1:]) + 1  # long after short
    at_c = np.flatnonzero(lg[:-1] & lg[1:])       # long before long
    at_d = at_c + 1                               # long after long
    if len(at_b):
        prev[at_b[rng.integers(0, len(at_b))]] = FLAG_BYTES[rng.integers(1, len(FLAG_BYTES))]
    if len(at_c):
        nxt[at_c[rng.integers(0, len(at_c))]] = 0
        prev[at_d[rng.integers(0, len(at_d))]] = 0
    if bs0 < bs1 and not allow_a:
        nxt[:-1][lg[:-1] & ~lg[1:]] = 0
    return prev, nxt


def window_flag_classes(blocks, prev, nxt):
    """-> dict class -> packet indices of one stream where its window flags disagree with the block flags around it:
    A long, next_long set, short block behind; B short, then long with prev_long set; C long with next_long clear, then long;
    D long, then long with prev_long clear. (A and B disagree only in name when blocksize0 == blocksize1.)"""
    b = np.asarray(blocks, np.uint8) == 1
    p = np.asarray(prev) != 0
    x = np.asarray(nxt) != 0
    out = dict(A=[], B=[], C=[], D=[])
    for i in range(len(b)):
        if not b[i]:
            continue
        if i + 1 < len(b) and x[i] and not b[i + 1]:
            out["A"].append(i)
        if i > 0 and not b[i - 1] and p[i]:
            out["B"].append(i)
        if i + 1 < len(b) and b[i + 1] and not x[i]:
            out["C"].append(i)
        if i > 0 and b[i - 1] and not p[i]:
            out["D"].append(i)
    return out


def _ogg_crc_table():
    t = []
    for i in range(256):
        r = i << 24
        for _ in range(8):
            r = ((r << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if r & 0x80000000 else (r << 1) & 0xFFFFFFFF
        t.append(r)
    return t


_OGG_CRC = _ogg_crc_table()


def ogg_crc(data):
    """Ogg page CRC (polynomial 0x04C11DB7, no reflection, initial value 0) of `data`, its CRC field zeroed by the caller."""
    c = 0
    for x in data:
        c = ((c << 8) & 0xFFFFFFFF) ^ _OGG_CRC[((c >> 24) & 0xFF) ^ x]
    return c


def fix_page_crcs(b):
    """Recompute, in place, the CRC of every complete page of the bytearray b, walking the pages as their segment tables lay them
    out, so that damage to a file reaches the codec layer instead of its CRC check. A torn page at the end is left as it is."""
    o = 0
    while o + 27 <= len(b) and b[o:o + 4] == b"OggS":
        ns = b[o + 26]
        if o + 27 + ns > len(b):
            break
        ln = 27 + ns + sum(b[o + 27:o + 27 + ns])
        if o + ln > len(b):
            break
        b[o + 22:o + 26] = b"\0\0\0\0"
        b[o + 22:o + 26] = ogg_crc(b[o:o + ln]).to_bytes(4, "little")
        o += ln
    return b


def ogg_pages(data):
    """-> [(offset, length, number of packets that end on the page)] of the complete pages at the start of data, in the walk of
    fix_page_crcs."""
    out = []
    o = 0
    while o + 27 <= len(data) and data[o:o + 4] == b"OggS":
        ns = data[o + 26]
        if o + 27 + ns > len(data):
            break
        lace = data[o + 27:o + 27 + ns]
        ln = 27 + ns + sum(lace)
        if o + ln > len(data):
            break
        out.append((o, ln, sum(1 for v in lace if v < 255)))
        o += ln
    return out


def sha256_bits(a):
    """sha256 hex digest of the bits of a float32 array (C order; callers keep the shape alongside)."""
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).view(np.uint32).tobytes()).hexdigest()


def fixture_setup(name):
    """SetupSpec of a committed .ogg fixture: test.stereo44khz / test.mono44khz (load_golden) or a stream of
    oracle/make_synth_ogg.py (synth_NN, winflags_*), whose .npz carries its synthesis-side setup."""
    if name.startswith("test."):
        return load_golden(name)[0]
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    floors = [(int(z["floor%d_mult" % k]), [int(x) for x in z["floor%d_xs" % k]]) for k in range(int(z["num_floors"]))]
    nmap = int(z["mode_mapping"].max()) + 1
    mappings = [([(int(a), int(b)) for a, b in z["coupling_m%d" % k]], [int(f) for f in z["chfloor_m%d" % k]]) for k in range(nmap)]
    modes = [(int(bf), int(mp)) for bf, mp in zip(z["mode_blockflag"], z["mode_mapping"])]
    return SetupSpec(int(z["channels"]), int(z["blocksize0"]), int(z["blocksize1"]), floors, mappings, modes)


def entropy_hook_digests(spec, d, upto):
    """sha256 of the "floor1 ys" and "after_residue" hooks of packets [0, upto) of an entropy dump (read_entropy_dump, float
    residue), in the form oracle/make_damaged_goldens.py records the reference's: per used channel (packet, channel, posts) + ys;
    per channel (packet, channel, n/2) + residue bits."""
    import hashlib
    ys, res = hashlib.sha256(), hashlib.sha256()
    C = spec.channels
    off = 0
    for p in range(min(upto, d["P"])):
        mode = int(d["packets"]["mode"][p])
        bf, mapping = spec.modes[mode]
        n2 = (spec.blocksize1 if bf else spec.blocksize0) // 2
        used = int(d["packets"]["floor_used"][p])
        for c in range(C):
            if (used >> c) & 1:
                posts = len(spec.floors[spec.mappings[mapping][1][c]][1])
                ys.update(np.asarray([p, c, posts], np.int32).tobytes() + d["ys"][p, c, :posts].astype(np.uint32).tobytes())
        for c in range(C):
            res.update(np.asarray([p, c, n2], np.int32).tobytes() + np.ascontiguousarray(d["residue"][off + c * n2:off + (c + 1) * n2]).tobytes())
        off += C * n2
    return ys.hexdigest(), res.hexdigest()


def load_damaged():
    """tests/golden/damaged.npz (oracle/make_damaged_goldens.py) -> list of dict per record."""
    z = np.load(os.path.join(GOLDEN, "damaged.npz"))
    names = [str(n) for n in z["base_names"]]
    recs = []
    for i in range(len(z["base"])):
        e0, e1 = int(z["edit_off"][i]), int(z["edit_off"][i + 1])
        recs.append(dict(index=i, seed=int(z["seed"][i]), draw=int(z["draw"][i]), base=names[int(z["base"][i])], kind=str(z["kind"][i]),
                         edit_pos=z["edit_pos"][e0:e1], edit_val=z["edit_val"][e0:e1], trunc=int(z["trunc"][i]),
                         sha=str(z["sha"][i]), ref_rc=int(z["ref_rc"][i]), ref_err=str(z["ref_err"][i]), ref_packets=int(z["ref_packets"][i]),
                         ref_frames=int(z["ref_frames"][i]), ref_pcm=str(z["ref_pcm"][i]), ref_ys=str(z["ref_ys"][i]),
                         ref_res=str(z["ref_res"][i]), expect_ok=bool(z["expect_ok"][i]), expect_flags=int(z["expect_flags"][i]),
                         expect_bad=int(z["expect_bad"][i]), hook_sha=str(z["hook_sha"][i]), hook_off=int(z["hook_off"][i]),
                         hook_num=int(z["hook_num"][i])))
    return recs, z


def damaged_bytes(rec):
    """Rebuild one damaged file of tests/golden/damaged.npz from its base fixture and recipe: byte edits, truncation, then every
    complete page's CRC recomputed. Asserts the sha256 the generator recorded."""
    import hashlib
    b = bytearray(open(os.path.join(GOLDEN, rec["base"] + ".ogg"), "rb").read())
    for p, v in zip(rec["edit_pos"], rec["edit_val"]):
        b[int(p)] = int(v)
    if rec["trunc"] >= 0:
        del b[rec["trunc"]:]
    fix_page_crcs(b)
    data = bytes(b)
    assert hashlib.sha256(data).hexdigest() == rec["sha"], (rec["base"], rec["seed"], rec["draw"])
    return data


def read_entropy_dump(path):
    """Parse the file written by tests/host_entropy_dump.cpp -> dict (packets, ys, residue, and in VQ mode vq_packets,
    cls, entries, residue_floats, vq_spec)."""
    from parseoggvorbis_amd.binding import PACKET_DTYPE, VQ_PACKET_DTYPE, VqSpec
    raw = open(path, "rb").read()
    P, Cn, stride, nres, bs0, bs1 = (int(x) for x in np.frombuffer(raw[:24], np.uint32))
    off = 24
    d = dict(P=P, channels=Cn, ys_stride=stride, blocksize0=bs0, blocksize1=bs1)
    d["packets"] = np.frombuffer(raw[off:off + 16 * P], PACKET_DTYPE).copy()
    off += 16 * P
    d["ys"] = np.frombuffer(raw[off:off + 2 * P * Cn * stride], np.uint16).reshape(P, Cn, stride).copy()
    off += 2 * P * Cn * stride
    d["residue"] = np.frombuffer(raw[off:off + 4 * nres], np.float32).copy()
    off += 4 * nres
    if off == len(raw):
        return d

    def u32():
        nonlocal off
        v = int(np.frombuffer(raw[off:off + 4], np.uint32)[0])
        off += 4
        return v

    assert u32() == 0x31305156
    nvq, ncls, nent, rfl = u32(), u32(), u32(), u32()
    d["vq_packets"] = np.frombuffer(raw[off:off + 16 * nvq], VQ_PACKET_DTYPE).copy()
    off += 16 * nvq
    d["cls"] = np.frombuffer(raw[off:off + ncls], np.uint8).copy()
    off += ncls
    d["entries"] = np.frombuffer(raw[off:off + 2 * nent], np.uint16).copy()
    off += 2 * nent
    d["residue_floats"] = rfl
    books = []
    for _ in range(u32()):
        dims, n, has = u32(), u32(), u32()
        tab = None
        if has:
            tab = np.frombuffer(raw[off:off + 4 * dims * n], np.float32).copy()
            off += 4 * dims * n
        books.append((dims, n, tab))
    residues = []
    for _ in range(u32()):
        r = dict(type=u32(), begin=u32(), end=u32(), partition_size=u32(), num_classifications=u32(), classwords=u32())
        nb = r["num_classifications"] * 8
        r["books"] = np.frombuffer(raw[off:off + 2 * nb], np.int16).copy()
        off += 2 * nb
        residues.append(r)
    maps = []
    for _ in range(u32()):
        ns = u32()
        mux = list(raw[off:off + Cn])
        off += Cn
        sres = list(raw[off:off + ns])
        off += ns
        maps.append((mux, sres))
    assert off == len(raw)
    d["vq_spec"] = VqSpec(books, residues, maps)
    return d


def build_probe(tmpdir, testing=False):
    """Compile tests/host_entropy_dump.cpp against the built host library (testing: the build with the fault injection of
    PARSEOGGVORBIS_TEST_FAIL_AT compiled in); returns the executable's path."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "parseoggvorbis_amd", "host")
    csrc = os.path.join(root, "parseoggvorbis_amd", "csrc")
    out = os.path.join(str(tmpdir), "host_entropy_dump" + ("_testing" if testing else ""))
    subprocess.run(["g++", "-std=c++17", "-O2", "-o", out, os.path.join(root, "tests", "host_entropy_dump.cpp"),
                    "-L" + host, "-lparseoggvorbis_amd" + ("_testing" if testing else ""), "-L" + csrc, "-lvorbis_synth_hip", "-Wl,-rpath," + host,
                    "-Wl,-rpath," + csrc, "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    return out


def vq_submap_shapes(vq_spec, mapping, channels, n2):
    """-> [(vectors, partitions)] of one packet with n2 bins per channel, one pair per submap that has channels, in submap order:
    the shape of the classification array each of them reads (format 2: one interleaved vector)."""
    mux, sres = vq_spec.mappings[mapping]
    out = []
    for s in range(len(sres)):
        nch = sum(1 for c in range(channels) if mux[c] == s)
        if not nch:
            continue
        r = vq_spec.residues[sres[s]]
        fmt2 = r["type"] == 2
        ln = nch * n2 if fmt2 else n2
        out.append((1 if fmt2 else nch, (min(r["end"], ln) - min(r["begin"], ln)) // r["partition_size"]))
    return out


def synth_vq_packet(vq_spec, mapping, channels, n2, used_mask, rng, classes=None):
    """Random but well-formed (cls, entries) of one packet for `mapping`, in the decode order of hpp:708-760.
    classes: chosen classifications instead of random ones, one array [vectors][partitions] (vq_submap_shapes) per submap that has
    channels - the way to hit an exact entry count; the entry numbers stay random."""
    mux, sres = vq_spec.mappings[mapping]
    cls_all, ent_all = [], []
    k = 0
    for s in range(len(sres)):
        chans = [c for c in range(channels) if mux[c] == s]
        if not chans:
            continue
        r = vq_spec.residues[sres[s]]
        fmt2 = r["type"] == 2
        vch = 1 if fmt2 else len(chans)
        ln = len(chans) * n2 if fmt2 else n2
        parts = (min(r["end"], ln) - min(r["begin"], ln)) // r["partition_size"]
        if classes is None:
            cls = rng.integers(0, r["num_classifications"], (vch, parts)).astype(np.uint8)
        else:
            cls = np.asarray(classes[k], np.uint8).reshape(vch, parts)
            assert int(cls.max(initial=0)) < r["num_classifications"]
        k += 1
        used = [True] if fmt2 else [bool((used_mask >> c) & 1) for c in chans]
        for ps in range(8):
            for pc in range(parts):
                for j in range(vch):
                    if not used[j]:
                        continue
                    book = int(r["books"][int(cls[j, pc]) * 8 + ps])
                    if book < 0:
                        continue
                    dims, n, _ = vq_spec.codebooks[book]
                    ent_all.append(rng.integers(0, n, r["partition_size"] // dims).astype(np.uint16))
        cls_all.append(cls.ravel())
    cls = np.concatenate(cls_all) if cls_all else np.zeros(0, np.uint8)
    ent = np.concatenate(ent_all) if ent_all else np.zeros(0, np.uint16)
    return cls, ent


def synthetic_vq_spec(channels=2, bs1=2048, seed=5):
    """A residue VQ setup in the shape of the stereo fixture's long-block residue (format 2, begin 0, end 1600 of 2048
    interleaved bins, partition 32, 10 classes, three cascade passes, vector lengths 8/4/2/1), with small-integer value
    tables. Mapping 0 (short blocks) and 1 (long blocks) share it. For benchmarks and tests that need codebooks without an
    .ogg file."""
    from parseoggvorbis_amd.binding import VqSpec
    rng = np.random.default_rng(seed)
    books = []
    for dims, n, amp in ((8, 256, 1), (4, 256, 2), (4, 81, 1), (2, 128, 3), (2, 64, 1), (1, 32, 8), (1, 16, 2)):
        tab = rng.integers(-amp, amp + 1, (n, dims)).astype(np.float32)
        tab[rng.random((n, dims)) < 0.5] = 0
        books.append((dims, n, tab.ravel()))
    nclass = 10
    cas = np.full((nclass, 8), -1, np.int16)
    cas[1, 0] = 0
    cas[2, 0], cas[2, 1] = 1, 4
    cas[3, 0] = 2
    cas[4, 0], cas[4, 1] = 3, 6
    cas[5, 1] = 4
    cas[6, 0], cas[6, 1], cas[6, 2] = 1, 3, 5
    cas[7, 2] = 6
    cas[8, 0], cas[8, 2] = 0, 5
    cas[9, 0], cas[9, 1], cas[9, 2] = 2, 4, 6
    n2 = bs1 // 2
    end = (channels * n2 * 25 // 32) // 32 * 32  # 1600 of 2048 for stereo 2048
    res = dict(type=2, begin=0, end=end, partition_size=32, num_classifications=nclass, classwords=2, books=cas.ravel())
    mux = [0] * channels
    return VqSpec(books, [res], [(mux, [0]), (mux, [0])])


def exotic_vq_spec(variant, channels=2, bs0=256, bs1=2048, seed=9):
    """Residue setups the fixtures do not have, for oracle-vs-device tests of the VQ stage:
    'format0'   one submap, residue format 0 (interleaved components, hpp:738-746), partition 16, vector lengths 2/4/8/16
    'format1x2' one submap holding both channels as two format-1 vectors (partition counter shared, hpp:726-757), partition 12,
                vector lengths 1/2/3/4/6 (not powers of two, partition not a multiple of 8: the general path and its tails),
                begin > 0 and end below the block
    'submaps'   channel 0 -> submap 0 (format 1), channel 1 -> submap 1 (format 0): two residues per packet"""
    from parseoggvorbis_amd.binding import VqSpec
    rng = np.random.default_rng(seed)

    def book(dims, n, amp):
        tab = rng.integers(-amp, amp + 1, (n, dims)).astype(np.float32)
        return (dims, n, tab.ravel())

    def cascade(nclass, nbooks, density):
        c = np.full((nclass, 8), -1, np.int16)
        for k in range(1, nclass):
            for ps in range(8):
                if rng.random() < density:
                    c[k, ps] = int(rng.integers(0, nbooks))
        return c.ravel()

    if variant == "format0":
        books = [book(2, 50, 3), book(4, 81, 2), book(8, 100, 1), book(16, 37, 1)]
        res = [dict(type=0, begin=0, end=bs1 // 2, partition_size=16, num_classifications=6, classwords=2, books=cascade(6, 4, 0.35))]
        maps = [([0] * channels, [0]), ([0] * channels, [0])]
    elif variant == "format1x2":
        books = [book(1, 9, 5), book(2, 25, 3), book(3, 27, 2), book(4, 40, 2), book(6, 64, 1)]
        res = [dict(type=1, begin=24, end=bs1 // 2 - 100, partition_size=12, num_classifications=7, classwords=3,
                    books=cascade(7, 5, 0.3))]
        maps = [([0] * channels, [0]), ([0] * channels, [0])]
    else:
        books = [book(1, 16, 4), book(2, 64, 2), book(4, 128, 2), book(8, 60, 1)]
        res = [dict(type=1, begin=0, end=bs1 // 2, partition_size=32, num_classifications=5, classwords=2, books=cascade(5, 4, 0.4)),
               dict(type=0, begin=8, end=bs1 // 4, partition_size=8, num_classifications=4, classwords=1, books=cascade(4, 4, 0.4))]
        mux = [i % 2 for i in range(channels)]
        maps = [(mux, [0, 1]), (mux, [0, 1])]
    # the class codebook's vector length only matters to the host's bit reader; books here always have a value table
    return VqSpec(books, res, maps)


def build_vq_spec(channels, mux, residues, submap_residues, seed=17):
    """A residue VQ setup from its shape, beside synthetic_vq_spec / exotic_vq_spec (whose outputs it leaves alone).
    mux: submap of every channel - one list for every mapping, or one list per mapping.
    residues: list of dict(type, partition_size, begin, end, dims=[vector length, ...]) with optional nclass (6), density (0.35: the
        chance that a (class, pass) pair has a book; class 0 has none) or cascade (an int [nclass][8] array of indices into dims,
        -1: no book, instead of a drawn one). Every residue gets books of its own, one per entry of dims.
    submap_residues: per mapping, the residue of each submap ([[0], [0]]: both mappings share residue 0).
    Value tables are float32 normal deviates scaled by powers of two that differ from book to book, so that every addition of the
    accumulation rounds and a sum taken in another order, or with a pass left out, differs in its bits."""
    from parseoggvorbis_amd.binding import VqSpec
    rng = np.random.default_rng(seed)
    books, res = [], []
    for r in residues:
        first = len(books)
        for k, dims in enumerate(r["dims"]):
            n = int(rng.integers(9, 140))
            tab = (rng.standard_normal((n, dims)) * 2.0 ** (k % 5 - 1)).astype(np.float32)
            books.append((dims, n, tab.ravel()))
        nclass = int(r.get("nclass", 6))
        if "cascade" in r:
            cas = np.asarray(r["cascade"], np.int64).reshape(nclass, 8)
        else:
            cas = np.full((nclass, 8), -1, np.int64)
            for c in range(1, nclass):
                for ps in range(8):
                    if rng.random() < r.get("density", 0.35):
                        cas[c, ps] = int(rng.integers(0, len(r["dims"])))
        cas = np.where(cas >= 0, cas + first, -1).astype(np.int16)
        res.append(dict(type=r["type"], begin=r["begin"], end=r["end"], partition_size=r["partition_size"], num_classifications=nclass,
                        classwords=2, books=cas.ravel()))
    per_map = mux if isinstance(mux[0], (list, tuple)) else [mux] * len(submap_residues)
    assert all(len(m) == channels for m in per_map)
    return VqSpec(books, res, [(list(m), list(sr)) for m, sr in zip(per_map, submap_residues)])


def propagated_used(spec, mode, own):
    """floor_used after the coupling step has brought both channels of a pair to life where either is (hpp:1174-1180)."""
    used = int(own)
    for mag, ang in spec.mappings[spec.modes[mode][1]][0]:
        if (used >> mag) & 1 or (used >> ang) & 1:
            used |= (1 << mag) | (1 << ang)
    return used


def vq_pool_packet(spec, vq_spec, mode, own, rng, classes=None):
    """One packet of mode `mode` for assemble_vq_batch: dict(long, mode, mapping, own, used, n2, cls, ent). own: the packet's
    floor_used; classes: see synth_vq_packet."""
    n2 = spec.blocksize_of_mode(mode) // 2
    used = propagated_used(spec, mode, own)
    mapping = spec.modes[mode][1]
    cls, ent = synth_vq_packet(vq_spec, mapping, spec.channels, n2, used, rng, classes)
    return dict(long=int(bool(spec.modes[mode][0])), mode=mode, mapping=mapping, own=int(own), used=used, n2=n2, cls=cls, ent=ent)


def random_own_mask(rng, channels, partial=0.3):
    """floor_used of a random packet: every channel, or (with probability `partial`) a random subset - the draw of
    tests/test_gpu_vq.py's batches."""
    return int(rng.integers(0, 1 << channels)) if rng.random() < partial else (1 << channels) - 1


def assemble_vq_batch(spec, pkts, streams, ent_mod8=None, bad_mode=()):
    """The VQ stage's batch from a list of pool packets (vq_pool_packet; the same dict may appear many times) in submit order, cut
    into `streams` equal segments that each start a stream. Window flags agree with the block sequence.
    ent_mod8[p]: packet p's entry_off modulo 8 (-1: wherever it falls), reached by putting entry numbers that no packet reads
        (0xFFFF) in front of its own.
    bad_mode: packets whose mode byte is replaced by one the setup does not have; the layout takes them for short blocks.
    -> dict(packets, segments, vq_packets, cls, entries, res_off [P + 1] (float index of every packet's residue), plane_stride)"""
    P = len(pkts)
    assert P % streams == 0
    per = P // streams
    pk = np.zeros(P, PACKET_DTYPE)
    from parseoggvorbis_amd.binding import VQ_PACKET_DTYPE
    vqp = np.zeros(P, VQ_PACKET_DTYPE)
    seg = np.zeros(streams, SEGMENT_DTYPE)
    res_off = np.zeros(P + 1, np.int64)
    cls_l, ent_l = [], []
    c_off = e_off = 0
    lng = [0 if p in bad_mode else k["long"] for p, k in enumerate(pkts)]
    for p, k in enumerate(pkts):
        q = p % per
        if q == 0:
            seg[p // per] = (p // per, p, per, VSYN_SEG_RESET, res_off[p])
        pk[p]["mode"], pk[p]["granule"], pk[p]["floor_used"] = (len(spec.modes) + 3 if p in bad_mode else k["mode"]), -1, k["own"]
        pk[p]["prev_long"] = lng[p - 1] if q else 1
        pk[p]["next_long"] = lng[p + 1] if q + 1 < per else 1
        if not lng[p]:
            pk[p]["prev_long"] = pk[p]["next_long"] = 1
        npad = (int(ent_mod8[p]) - e_off) % 8 if ent_mod8 is not None and ent_mod8[p] >= 0 else 0
        if npad:
            ent_l.append(np.full(npad, 0xFFFF, np.uint16))
            e_off += npad
        vqp[p] = (e_off, k["ent"].size, c_off)
        cls_l.append(k["cls"])
        ent_l.append(k["ent"])
        c_off += k["cls"].size
        e_off += k["ent"].size
        res_off[p + 1] = res_off[p] + spec.channels * (spec.blocksize0 // 2 if p in bad_mode else k["n2"])
    return dict(packets=pk, segments=seg, vq_packets=vqp, cls=np.concatenate(cls_l + [np.zeros(0, np.uint8)]),
                entries=np.concatenate(ent_l + [np.zeros(0, np.uint16)]), res_off=res_off, plane_stride=per * (spec.blocksize1 // 2) + 64)
