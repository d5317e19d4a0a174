"""The residue VQ setups of tests/test_gpu_vq_shapes.py (the kernel against the oracle) and tests/test_vq_model_cpu.py (the oracle
against tests/vq_model.py), built with tests/workloads.build_vq_spec. numpy only; every function is deterministic."""
import numpy as np

from parseoggvorbis_amd.binding import SetupSpec
from tests.workloads import build_vq_spec, fixture_like_spec, random_own_mask, vq_pool_packet, vq_submap_shapes


def stream_spec(channels, bs0, bs1, couplings=(), modes=((0, 0), (1, 1))):
    """Stream setup for `channels` channels: the fixtures' floors scaled to the block pair, every mapping with `couplings`, one
    mapping per distinct mapping number in `modes` (short-block mappings use floor 0, the others floor 1)."""
    f = fixture_like_spec(channels, bs0, bs1, coupled=False)
    nmap = max(m for _, m in modes) + 1
    long_maps = {m for bf, m in modes if bf}
    mappings = [(list(couplings), [1 if m in long_maps else 0] * channels) for m in range(nmap)]
    return SetupSpec(channels, bs0, bs1, f.floors, mappings, [tuple(m) for m in modes])


# ---- a. channels x formats at 128/1024 (n2 = 64 / 512) --------------------------------------------------------------------------
# name -> (channels, couplings, mux, residues, submap residues). Every setup keeps 8 * parts * vectors <= 8192.
# The format 2 ones: begin and begin + parts * psize are no multiples of the channel count on long blocks (checked by
# test_vq_model_cpu), begin is odd in f2x3 / f2x5 and 2 mod 4 in f2x6; the format 0 / 1 ones have begin = 1, 2, 3 mod 4.
CHANNEL_CASES = {
    "f2x3": (3, [], [0, 0, 0], [dict(type=2, partition_size=16, begin=7, end=1500, dims=[1, 2, 4, 8, 16])], [[0], [0]]),
    "f2x5": (5, [], [0] * 5, [dict(type=2, partition_size=24, begin=11, end=2500, dims=[1, 2, 4, 8, 3])], [[0], [0]]),
    "f2x6": (6, [], [0] * 6, [dict(type=2, partition_size=20, begin=4, end=3000, dims=[1, 2, 4, 5, 10])], [[0], [0]]),
    "f2x2odd": (2, [(0, 1)], [0, 0], [dict(type=2, partition_size=16, begin=5, end=120, dims=[1, 2, 4, 8]),
                                      dict(type=2, partition_size=16, begin=6, end=1000, dims=[1, 2, 4, 8, 16])], [[0], [1]]),
    "f1x3": (3, [], [0, 0, 0], [dict(type=1, partition_size=16, begin=5, end=500, dims=[1, 2, 4, 8])], [[0], [0]]),
    "f1x6": (6, [], [0] * 6, [dict(type=1, partition_size=12, begin=6, end=400, dims=[1, 2, 3, 4, 6], nclass=9)], [[0], [0]]),
    "f0x3": (3, [], [0, 0, 0], [dict(type=0, partition_size=16, begin=3, end=512, dims=[2, 4, 8, 16])], [[0], [0]]),
    "f0x6": (6, [], [0] * 6, [dict(type=0, partition_size=8, begin=0, end=300, dims=[1, 2, 4, 8])], [[0], [0]]),
    # the 5.1 shape: five channels interleaved in format 2, the LFE channel (3) alone in format 1
    "5.1": (6, [(0, 1), (4, 5)], [0, 0, 0, 1, 0, 0], [dict(type=2, partition_size=32, begin=0, end=2400, dims=[1, 2, 4, 8]),
                                                      dict(type=1, partition_size=8, begin=0, end=64, dims=[1, 2, 4])], [[0, 1], [0, 1]]),
    # chained couplings: a packet whose own mask is {2} decodes channels 1 and 2 and not 0 (the pairs are walked once, in order)
    "chain3": (3, [(0, 1), (1, 2)], [0, 0, 0], [dict(type=1, partition_size=8, begin=3, end=490, dims=[1, 2, 4, 8])], [[0], [0]]),
}


def channel_case(name, seed=3):
    C, coup, mux, residues, sres = CHANNEL_CASES[name]
    return stream_spec(C, 128, 1024, coup), build_vq_spec(C, mux, residues, sres, seed=seed)


# ---- b. block sizes, stereo ---------------------------------------------------------------------------------------------------
BLOCK_PAIRS = [(64, 8192), (64, 64), (4096, 4096), (512, 4096)]


def block_case(bs0, bs1, extra_partition=False):
    """Stereo. Short blocks (mapping 0): channel 0 and 1 in a submap each. At n2 = 32 the first residue begins behind the vector
    (no partition, no entry: the channel is zero fill only) and the second holds exactly one partition; at other sizes they are a
    format 1 and a format 0 residue with odd begins. Long blocks (mapping 1): both channels in one format 2 submap; at 8192 with
    partition 8 over the whole vector = 1024 partitions = 8192 slots (VQ_MAX_SLOTS: 16 rounds of the scan, each with carries).
    extra_partition: the long residue in partitions of 4 over 4100 elements instead, 1025 partitions - one more than the stage takes."""
    n2s, n2l = bs0 // 2, bs1 // 2
    if n2s == 32:
        short = [dict(type=1, partition_size=8, begin=40, end=56, dims=[1, 2, 4, 8]),
                 dict(type=1, partition_size=16, begin=9, end=31, dims=[1, 2, 4, 8, 16])]
    else:
        short = [dict(type=1, partition_size=16, begin=3, end=n2s - 5, dims=[1, 2, 4, 8]),
                 dict(type=0, partition_size=8, begin=5, end=n2s, dims=[1, 2, 4, 8])]
    if extra_partition:
        long_ = dict(type=2, partition_size=4, begin=0, end=4100, dims=[1, 2, 4])
    elif bs1 == 8192:
        long_ = dict(type=2, partition_size=8, begin=0, end=8192, dims=[1, 2, 4, 8], nclass=5)
    else:
        long_ = dict(type=2, partition_size=32, begin=1, end=2 * n2l - 3, dims=[1, 2, 4, 8, 16, 32])
    return (stream_spec(2, bs0, bs1, [(0, 1)]),
            build_vq_spec(2, [[0, 1], [0, 0]], short + [long_], [[0, 1], [2]], seed=bs0 + bs1))


# ---- c. the packet walk -------------------------------------------------------------------------------------------------------
# modes of the walk setups: name -> mode number
WALK_MODES = dict(SA=0, LA=1, LBC=2, LB=3)


def walk_case(tables_in_lds):
    """Stereo 128/1024 with three mappings, for tests that make one wave decode packet after packet:
      mapping 0  one submap, residue A (format 2, 10 classes; class 9 costs 48 entries per partition: 3072 per long block)
      mapping 1  two submaps: channel 1 -> submap 0 -> residue B, channel 0 -> submap 1 -> residue C (crossed, so that submap 0 of
                 this mapping and submap 0 of the others do not start with the same channel: a channel list kept from another
                 mapping, or from the other submap, stores into the wrong channel)
      mapping 2  one submap, residue B (format 1, both channels side by side)
    and four modes: SA (short, mapping 0), LA (long, mapping 0), LBC (long, mapping 1), LB (long, mapping 2).
    tables_in_lds: B and C are format 1 with power-of-two vector lengths and partitions of 8 / 16 and every book is small, so that
    the setup is eligible for the kernel that keeps the value tables in LDS; otherwise B has partitions of 12 with vector lengths 3
    and 6 and C is format 0, which need the general route and keep the tables in global memory."""
    cas_a = np.full((10, 8), -1, np.int64)  # indices into dims = [8, 4, 2, 1]
    cas_a[1, 0] = 0
    cas_a[2, 0], cas_a[2, 1] = 1, 2
    cas_a[3, 1] = 1
    cas_a[4, 0], cas_a[4, 2] = 2, 3
    cas_a[5, 2] = 0
    cas_a[6, 0], cas_a[6, 1], cas_a[6, 2] = 0, 1, 2
    cas_a[7, 3] = 2
    cas_a[8, 0], cas_a[8, 5] = 1, 0
    cas_a[9, 0], cas_a[9, 1], cas_a[9, 2] = 3, 3, 3
    a = dict(type=2, partition_size=16, begin=0, end=1024, dims=[8, 4, 2, 1], nclass=10, cascade=cas_a)
    if tables_in_lds:
        b = dict(type=1, partition_size=8, begin=8, end=500, dims=[1, 2, 4, 8], nclass=5, density=0.4)
        c = dict(type=1, partition_size=16, begin=0, end=480, dims=[2, 4, 16], nclass=3, density=0.5)
    else:
        b = dict(type=1, partition_size=12, begin=8, end=500, dims=[1, 2, 3, 4, 6], nclass=5, density=0.4)
        c = dict(type=0, partition_size=16, begin=0, end=480, dims=[2, 4, 16], nclass=3, density=0.5)
    spec = stream_spec(2, 128, 1024, [(0, 1)], modes=((0, 0), (1, 0), (1, 1), (1, 2)))
    return spec, build_vq_spec(2, [[0, 0], [1, 0], [0, 0]], [a, b, c], [[0], [1, 2], [1]], seed=77)


WALK_LIGHT = [0, 1, 2, 3, 4, 5, 6, 7, 8]  # classes of residue A that keep a long block at or below 64 * 28 = 1792 entries
WALK_TOUR = ["LA", "SA", "LA", "LB", "LA", "LBC", "LA", "BIG", "ZERO", "LA", "BAD", "LA"]


def walk_packet(spec, vqs, kind, rng):
    """One packet of the walk: SA / LA / LB / LBC random packets of those modes (residue A restricted to WALK_LIGHT: at most 2048
    entries, at least one); BIG a long block of mode LA with 3072 entries (read from global memory), ZERO one with no entry at all;
    BAD is an LA packet that assemble_vq_batch's bad_mode then spoils."""
    own = random_own_mask(rng, 2)
    if kind in ("LB", "LBC"):
        return vq_pool_packet(spec, vqs, WALK_MODES[kind], own, rng)
    mode = WALK_MODES["SA" if kind == "SA" else "LA"]
    (_, parts), = vq_submap_shapes(vqs, spec.modes[mode][1], 2, spec.blocksize_of_mode(mode) // 2)
    if kind == "BIG":
        classes = np.full((1, parts), 9)
    elif kind == "ZERO":
        classes = np.zeros((1, parts), np.int64)
    else:
        classes = rng.choice(WALK_LIGHT, (1, parts))
        classes[0, 0] = 6  # never empty
    return vq_pool_packet(spec, vqs, mode, own, rng, [classes])


# ---- d. entry staging ---------------------------------------------------------------------------------------------------------
# synthetic_vq_spec(2, 2048): 50 partitions of a long block; its classes cost 0, 4, 24, 8, 48, 16, 56, 32, 36, 56 entries each.
# entry count -> {class: partitions}; the other partitions are class 0. 2048 is VQ_ENT_CAP, the most that is staged in LDS.
STAGING_COUNTS = {2044: {6: 18, 9: 17, 4: 1, 8: 1},   # 35 * 56 + 48 + 36
                  2048: {6: 18, 9: 18, 7: 1},         # 36 * 56 + 32
                  2052: {6: 18, 9: 18, 8: 1}}         # 36 * 56 + 36


def staging_classes(counts, rng, parts=50):
    cls = np.zeros(parts, np.int64)
    at = 0
    for c, k in counts.items():
        cls[at:at + k] = c
        at += k
    rng.shuffle(cls)
    return cls.reshape(1, parts)


# ---- e. packed counts near 16 bits --------------------------------------------------------------------------------------------
def packed_counts_case(channels, partition_size, fmt=2):
    """`channels` uncoupled channels at 8192/8192 in one format 2 submap over [0, 61440): every class has a vector-length-1 book in
    passes 0 and 1 and a length-2 book in pass 2, so passes 0 and 1 each hold 61 440 entries - both 16-bit halves of one word of
    the kernel's packed scan end just below 65 536. fmt=1: the channels side by side as format 1 vectors over [0, 4096) instead;
    a pass holds the entries of all of them, the same 4096 per channel."""
    nclass = 3
    cas = np.full((nclass, 8), -1, np.int64)  # indices into dims = [1, 1, 1, 2, 2]
    cas[0, :3] = (0, 1, 3)
    cas[1, :3] = (1, 2, 4)
    cas[2, :3] = (2, 0, 3)
    r = dict(type=fmt, partition_size=partition_size, begin=0, end=61440 if fmt == 2 else 4096, dims=[1, 1, 1, 2, 2], nclass=nclass,
             cascade=cas)
    return stream_spec(channels, 8192, 8192), build_vq_spec(channels, [0] * channels, [r], [[0], [0]], seed=channels)


# ---- every setup above, for the model-against-oracle test ---------------------------------------------------------------------
def all_cases():
    """name -> (SetupSpec, VqSpec) of every setup of this file that the stage accepts."""
    out = {"channels/" + n: channel_case(n) for n in CHANNEL_CASES}
    for bs0, bs1 in BLOCK_PAIRS:
        out["blocks/%d_%d" % (bs0, bs1)] = block_case(bs0, bs1)
    out["walk/global"] = walk_case(False)
    out["walk/lds"] = walk_case(True)
    out["packed/64"] = packed_counts_case(15, 64)
    out["packed/60"] = packed_counts_case(15, 60)
    out["packed/format1"] = packed_counts_case(15, 64, fmt=1)
    return out
