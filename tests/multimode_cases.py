"""Stream setups with several modes per block size, a floor per channel and table numbers up to 63, as ONE seeded case table for
test_multimode_cpu.py and test_gpu_multimode.py. numpy only, no GPU.

Every other synthesis test keeps "floor 0 = short blocks, floor 1 = long blocks, every channel of a mapping on the same floor"; the
geometry cases have eight modes that share one X list per block size. Vorbis I allows 64 floors, mappings and modes, a floor per
channel and any mode number for any block size, and the device caches exactly what those setups never move: the lane constants of
the current floor (vsyn_fused.h: cur_map / map_floor / cur_floor, the prefetched coded row), the mapping of a packed pass (both
fused kernels), the floors of a wave of rows (floor1_unwrap_rows) and the modes of a wave of packets (vsyn_prep.h, the 64-bit
long_modes bitmap and the mode_mapping dwords).

X lists come from a seeded pool per block-size pair: x[0] = 0, x[1] = half the floor's block, the inner posts distinct and in
shuffled header order. Post counts sit at the code's thresholds: 2 (no inner post), 9, 32 (the largest register form of
floor1_unwrap_rows), 33 (its first LDS form), 64 (the tuned kernel's limit) and 65 (VSYN_MAX_POSTS, the size-generic kernel only);
a short floor has at most bs0 / 2 + 1 distinct X. No two floors of a setup share a post count (numbering: no two floors that a
packet uses — 64 floors of at most 64 posts, two at least, cannot all differ), and neighbouring modes differ in multiplier.

Cases (CASES; every one gives a "mixed" batch, L L L S*8 rotated per stream, and a "long" batch):
  long_modes          stereo 256/2048, [(0, 1)] in every mapping: short modes of 9 and 2 posts, long modes of 12, 32 and 64 posts;
                      mode k -> mapping (k + 2) % 5 -> floor (k + 4) % 5, so that no table index equals another. Tuned kernel.
  long_modes_u        the same with long floors of 12, 33 and 65 posts on the size-generic kernel: 128/1024 and 512/4096 stereo
                      (register sets), 64/256 mono (eight packets a pass at either size: a mapping change inside a pass)
  channel_floors      mappings whose channels use different floors: stereo [f32, f33] in one long mode, [f33, f32] in another and
                      [f12, f64] in a third (adjacent rows of the unwrap alternate between the register and the LDS form); three
                      channels [fa, fb, fa] with couplings [(0, 1), (1, 2)] (the size-generic kernel's general replay, role 3). At
                      256/2048 and 128/1024, a quarter of the channels unused.
  numbering           64 modes, 64 mappings, 64 floors. Mode 0 is LONG; packets use modes 0 1 3 4 31 32 33 62 63 (long: 0 3 32 62),
                      mode 63 -> mapping 63 -> floor 63, every other mode k -> mapping 62 - k -> floor (79 - k) % 63. Mono and stereo,
                      128/1024 and 256/2048; uncoupled or [(0, 1)] throughout.
  couplings_disagree  stereo 256/2048, two long modes whose mappings carry [(0, 1)] and [(1, 0)] (variant "swapped") or [(0, 1)] and
                      [] (variant "none"). By the dispatch rules: fused_coupling_mode finds long-mode mappings that disagree (-1), so
                      fused_setup_ok and with it fused_ok_mask give 0; u_supported holds (two channels, no floor above 65 posts), so
                      vsyn_create hands every run to the size-generic kernel (vsyn_fused_paths & 3 == 2) with u_role_mode 3, the
                      general replay. The tuned kernel must NOT run: it has one coupling role per wave.

Mode patterns. long: stream 0 changes the long mode at every packet, stream 1 at every second packet, stream 2 once on packet 11
(the halo of the run that starts at 12, for run lengths 3 and 4) and once on packet 24 (a run's first packet for both). mixed:
stream 0 alternates the short modes packet by packet (the stretch of eight ends on the other mode than the next one starts with, so
the short mode also changes exactly at a long/short transition) and cycles the long modes; stream 1 changes the short mode every
fourth packet and the long mode every second long packet."""
import numpy as np

from parseoggvorbis_amd.binding import SetupSpec
from tests.workloads import synth_batch

LONG_STREAMS, LONG_PACKETS = 3, 48
MIXED_STREAMS, MIXED_PACKETS = 2, 44
TUNED = (3, "vsyn_fused_kernel", "vsyn_fused_tap_kernel")
GENERIC = (2, "vsyn_fused_u_kernel", "vsyn_fused_u_tap_kernel")
NUMBERING_USED = (0, 1, 3, 4, 31, 32, 33, 62, 63)
NUMBERING_LONG = (0, 3, 32, 62)


def pool_xs(rng, h, posts):
    """An X list of `posts` posts for a block of half size h: [0, h] and posts - 2 distinct inner X in shuffled header order"""
    assert 2 <= posts <= h + 1, (posts, h)
    inner = [int(v) for v in rng.choice(np.arange(1, h), posts - 2, replace=False)] if posts > 2 else []
    if len(inner) > 1 and inner == sorted(inner):  # (a short draw can come out sorted)
        inner = inner[1:] + inner[:1]
    return [0, h] + inner


def _floors(rng, bs0, bs1, desc):
    """desc: [(long, posts, multiplier)] in floor order -> [(multiplier, xs)]"""
    return [(mult, pool_xs(rng, (bs1 if lng else bs0) // 2, posts)) for lng, posts, mult in desc]


def _rng(case, bs0, bs1, channels):
    return np.random.default_rng([sorted(BUILDERS).index(case), bs0, bs1, channels])


def _long_modes(case, bs0, bs1, channels, big):
    """modes S9 L12 Lmid S2 Lbig; mode k -> mapping (k + 2) % 5 -> floor (k + 4) % 5"""
    mid = 32 if big == 64 else 33
    by_mode = [(0, 9, 4), (1, 12, 2), (1, mid, 1), (0, 2, 3), (1, big, 4)]
    fdesc = [None] * 5
    mappings = [None] * 5
    coup = [(0, 1)] if channels == 2 else []
    for k, d in enumerate(by_mode):
        fdesc[(k + 4) % 5] = d
        mappings[(k + 2) % 5] = (coup, [(k + 4) % 5] * channels)
    modes = [(d[0], (k + 2) % 5) for k, d in enumerate(by_mode)]
    spec = SetupSpec(channels, bs0, bs1, _floors(_rng(case, bs0, bs1, channels), bs0, bs1, fdesc), mappings, modes)
    return spec, [1, 2, 4], [0, 3]


def _channel_floors(case, bs0, bs1, channels, big):
    """floors 0..5: L32 S9 L33 L12 S2 Lbig; stereo long modes [f32, f33] / [f33, f32] / [f12, fbig], short [f9, f2] / [f2, f9];
    three channels [fa, fb, fa] with the same pairs"""
    fdesc = [(1, 32, 2), (0, 9, 4), (1, 33, 1), (1, 12, 3), (0, 2, 1), (1, big, 2)]
    pairs = [(0, 2), (2, 0), (3, 5), (1, 4), (4, 1)]  # (fa, fb) per mapping
    coup = [(0, 1)] if channels == 2 else [(0, 1), (1, 2)]
    mappings = [(coup, [a, b] if channels == 2 else [a, b, a]) for a, b in pairs]
    modes = [(0, 3), (1, 1), (1, 2), (0, 4), (1, 0)]  # S[f9 f2]  L[f33 f32]  L[f12 fbig]  S[f2 f9]  L[f32 f33]
    spec = SetupSpec(channels, bs0, bs1, _floors(_rng(case, bs0, bs1, channels), bs0, bs1, fdesc), mappings, modes)
    return spec, [4, 1, 2], [0, 3]


def _numbering(case, bs0, bs1, channels, big):
    rng = _rng(case, bs0, bs1, channels)
    used_posts = {0: big, 3: 33, 32: 32, 62: 12, 1: 9, 4: 2, 31: 17, 33: 40, 63: 5}
    flag = [1 if k in NUMBERING_LONG else 0 if k in NUMBERING_USED else k % 2 for k in range(64)]
    mapping_of = [62 - k if k < 63 else 63 for k in range(64)]
    floor_of = [(m + 17) % 63 if m < 63 else 63 for m in range(64)]
    coup = [(0, 1)] if channels == 2 else []
    fdesc = [None] * 64
    for k in range(64):
        posts = used_posts.get(k, 3 + (k * 7) % 26)
        fdesc[floor_of[mapping_of[k]]] = (flag[k], posts, 1 + (k + k // 4) % 4)
    mappings = [(coup, [floor_of[m]] * channels) for m in range(64)]
    modes = [(flag[k], mapping_of[k]) for k in range(64)]
    spec = SetupSpec(channels, bs0, bs1, _floors(rng, bs0, bs1, fdesc), mappings, modes)
    return spec, list(NUMBERING_LONG), [k for k in NUMBERING_USED if k not in NUMBERING_LONG]


def _couplings_disagree(case, bs0, bs1, channels, variant):
    fdesc = [(1, 32, 2), (0, 9, 4), (1, 12, 1)]
    other = [(1, 0)] if variant == "swapped" else []
    mappings = [([(0, 1)], [1, 1]), ([(0, 1)], [2, 2]), (other, [0, 0])]
    modes = [(1, 2), (0, 0), (1, 1)]  # L32 with the other coupling, S9, L12 with [(0, 1)]
    spec = SetupSpec(2, bs0, bs1, _floors(_rng(case, bs0, bs1, 2 if variant == "swapped" else 3), bs0, bs1, fdesc), mappings, modes)
    return spec, [2, 0], [1]


BUILDERS = dict(long_modes=_long_modes, long_modes_u=_long_modes, channel_floors=_channel_floors, numbering=_numbering,
                couplings_disagree=_couplings_disagree)

# (case, bs0, bs1, channels, variant) -> (vsyn_fused_paths & 3, plain kernel, tap kernel) the dispatch rules give. variant: the
# post count of the largest long floor, or the second coupling of couplings_disagree.
CASES = {
    ("long_modes", 256, 2048, 2, 64): TUNED,
    ("long_modes_u", 128, 1024, 2, 65): GENERIC,
    ("long_modes_u", 512, 4096, 2, 65): GENERIC,
    ("long_modes_u", 64, 256, 1, 65): GENERIC,
    ("channel_floors", 256, 2048, 2, 64): TUNED,
    ("channel_floors", 128, 1024, 2, 65): GENERIC,
    ("channel_floors", 256, 2048, 3, 65): GENERIC,   # three channels: not the tuned kernel's (fused_supported)
    ("channel_floors", 128, 1024, 3, 65): GENERIC,
    ("numbering", 256, 2048, 2, 64): TUNED,
    ("numbering", 256, 2048, 1, 64): TUNED,
    ("numbering", 128, 1024, 2, 65): GENERIC,
    ("numbering", 128, 1024, 1, 65): GENERIC,
    ("couplings_disagree", 256, 2048, 2, "swapped"): GENERIC,
    ("couplings_disagree", 256, 2048, 2, "none"): GENERIC,
}
# channels for which a case promises consecutive packets of one block size on floors of different post counts
CLAIMS = {key: tuple(range(key[3])) for key in CASES}
UNUSED_FRAC = {"channel_floors": 0.25}


def case_id(key):
    return "%s-%d-%d-%dch-%s" % key


def make_setup(key):
    """-> (spec, long modes, short modes): the modes the case's packets use, in the order the patterns cycle them"""
    case, bs0, bs1, channels, variant = key
    return BUILDERS[case](case, bs0, bs1, channels, variant)


def long_pattern(longs):
    """-> modes(stream, q) of the all-long batch"""
    nl = len(longs)

    def modes(s, q):
        if s == 0:
            return longs[q % nl]
        if s == 1:
            return longs[(q // 2) % nl]
        return longs[0] if q < 11 else longs[nl - 1] if q < 24 else longs[1 if nl > 2 else 0]
    return modes


def mixed_pattern(longs, shorts, streams=MIXED_STREAMS, npk=MIXED_PACKETS):
    """-> [streams][npk] modes: block flags L L L S*8 rotated per stream as synth_batch's mixed pattern"""
    unit = [1, 1, 1] + [0] * 8
    flags1 = np.array((unit * (npk // len(unit) + 1))[:npk], np.uint8)
    out = []
    for s in range(streams):
        flags = np.roll(flags1, s % 11)
        cl = cs = 0
        row = []
        for q in range(npk):
            if flags[q]:
                row.append(longs[(cl if s % 2 == 0 else cl // 2) % len(longs)])
                cl += 1
            else:
                row.append(shorts[(cs if s % 2 == 0 else cs // 4) % len(shorts)])
                cs += 1
        out.append(row)
    return out


_BATCHES = {}


def batches(key):
    """-> (spec, {"mixed": batch, "long": batch}) of a case, built once per process and never written to"""
    if key not in _BATCHES:
        spec, longs, shorts = make_setup(key)
        seed = 7000 + sorted(CASES, key=case_id).index(key)
        uf = UNUSED_FRAC.get(key[0], 0.0)
        mixed = synth_batch(spec, MIXED_STREAMS, MIXED_PACKETS, seed=seed, unused_frac=uf, granule_last=True,
                            modes=np.array(mixed_pattern(longs, shorts)).ravel())
        lng = synth_batch(spec, LONG_STREAMS, LONG_PACKETS, seed=seed + 100, unused_frac=uf, granule_last=True, modes=long_pattern(longs))
        _BATCHES[key] = (spec, dict(mixed=mixed, long=lng))
    return _BATCHES[key]


def row_posts(spec, b):
    """-> int [P][C]: the post count of the floor of every (packet, channel) row"""
    return np.array([[len(spec.floors[spec.mappings[spec.modes[int(m)][1]][1][c]][1]) for c in range(spec.channels)]
                     for m in b["packets"]["mode"]])


def row_floors(spec, b):
    """-> int [P][C]: the floor number of every (packet, channel) row"""
    return np.array([[spec.mappings[spec.modes[int(m)][1]][1][c] for c in range(spec.channels)] for m in b["packets"]["mode"]])


def ring_groups(streams, npk, run_len, channels=2):
    """The tuned kernel's workgroups (16 waves: 8 runs x 2 channels) of an all-long stereo batch that take ring mode: all of the
    group's units lie in one segment (vsyn_fused.h, ring_ok). -> [(segment, first run)]"""
    per_seg = (npk + run_len - 1) // run_len * channels
    out = []
    for u0 in range(0, streams * per_seg, 16):
        if u0 // per_seg == (u0 + 15) // per_seg and (u0 + 15) // per_seg < streams:
            out.append((u0 // per_seg, (u0 % per_seg) // channels))
    return out
