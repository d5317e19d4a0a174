"""Generate tests/golden/features_<file>.npz: the reference's own RETURNN feature matrices for the committed .ogg fixtures.

Runs where the reference tree exists (authoring machines), after __graft_entry__.build() has built oracle/_ref/ours.bin:
  1. ours.bin --in <file>.ogg --debug_out <dump>   (the reference decoder; the dump holds every hook)
  2. the dump filtered to the hook names that returnn_import.py:84-113 passes for the kind (an unfiltered "floor1 ys" would
     add rows to the floor kinds)
  3. the reference's CallbacksOutputReader (demo_live_extract.py) over the filtered stream, imported with a stub `cffi` module
     (the reader does not use it), read_floor_ys / read_residue_ys with each grid entry's keyword arguments.
Each npz holds `grid` (JSON: [kind, output_dim, kwargs] per entry) and per entry `c<i>` (the matrix) or `e<i>` (the text of
the exception the reference raised). Only output data enters the repository.
Usage: python tools/make_feature_goldens.py [--ref /path/to/reference] [names...]"""
import argparse
import io
import json
import os
import struct
import subprocess
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = ["test.stereo44khz", "test.mono44khz"] + ["synth_%02d" % i for i in range(16)] + ["winflags_bcd"]

# (kind, output_dim, kwargs): the fixed grid the tests compare against
GRID = [
    ("floor_final_ys", 10, {}),
    ("floor_final_ys", 40, {}),
    ("floor_final_ys", 30, {"only_biggest_floor": True}),
    ("floor_final_ys", 20, {"include_floor_number": False, "floor_always_positive": True}),
    ("floor_final_ys_rendered", 40, {}),
    ("floor_final_ys_rendered", 30, {"sorted_xs": True}),
    ("floor_final_ys_rendered", 64, {"xs_from_biggest_floor": True}),
    ("floor_final_ys_rendered", 50, {"upscale_xs_factor": 2, "sorted_xs": True}),
    ("floor_final_ys_rendered", 30, {"only_biggest_floor": True, "upscale_xs_factor": 2, "xs_from_biggest_floor": True,
                                     "floor_always_positive": True}),
    ("floor_final_ys_rendered", 1, {"include_floor_number": False}),
    ("residue_ys", 70, {}),
    ("residue_ys", 70, {"log1p_abs_space": True, "scale": 0.5, "clip_abs_max": 0.8, "sorted_xs": True}),
    ("residue_ys", 40, {"ignore_xs": True}),
    ("residue_ys_with_floor", 70, {}),
    ("residue_ys_with_floor", 70, {"log1p_abs_space": True, "floor_base_factor": 2}),
    ("residue_ys_with_floor", 48, {"ignore_xs": True, "scale": 2.0, "clip_abs_max": 1.5}),
]

FILTERS = {  # returnn_import.py:84-113
    "floor_final_ys": ["floor_number", "floor1 final_ys"],
    "floor_final_ys_rendered": ["floor_number", "floor1 floor"],
    "residue_ys": ["floor_number", "after_residue"],
    "residue_ys_with_floor": ["floor_number", "floor1 floor", "after_residue"],
}
SETUP_NAMES = ["floor1_unpack multiplier", "floor1_unpack xs", "finish_setup"]
END_NAMES = ["finish_audio_packet"]


def split_records(raw):
    """the dump as (header bytes, [entry bytes]) — write_to_file records: key, type, elem size, data (each length-prefixed)"""
    off = 0

    def rec():
        nonlocal off
        n, = struct.unpack_from("I", raw, off)
        v = raw[off + 4:off + 4 + n]
        off += 4 + n
        return v

    def kv():
        start = off
        key = rec().decode()
        rec()
        rec()
        data = rec()
        return key, data, raw[start:off]

    rec()  # "ParseOggVorbis-header-v1"
    for _ in range(3):
        kv()
    header = raw[:off]
    entries = []
    while off < len(raw):
        start = off
        key, name, _ = kv()
        assert key == "entry-name", key
        key, data, _ = kv()
        if key == "entry-channel":
            key, data, _ = kv()
        assert key == "entry-data"
        entries.append((name.decode(), raw[start:off]))
    return header, entries


def load_reader_class(ref):
    sys.modules.setdefault("cffi", types.ModuleType("cffi"))  # imported at module level, unused by the reader
    parent = os.path.dirname(os.path.abspath(ref))
    if parent not in sys.path:
        sys.path.insert(0, parent)
    import importlib
    mod = importlib.import_module(os.path.basename(os.path.abspath(ref)) + ".demo_live_extract")
    return mod.CallbacksOutputReader


def make(name, reader_cls, ours):
    ogg = os.path.join(GOLDEN, name + ".ogg")
    with tempfile.TemporaryDirectory() as td:
        dump = os.path.join(td, "dump.bin")
        subprocess.run([ours, "--in", ogg, "--debug_out", dump], check=True, stdout=subprocess.DEVNULL)
        raw = open(dump, "rb").read()
    header, entries = split_records(raw)
    out = {"grid": np.array(json.dumps(GRID))}
    for i, (kind, dim, kw) in enumerate(GRID):
        keep = set(SETUP_NAMES + FILTERS[kind] + END_NAMES)
        stream = header + b"".join(b for nm, b in entries if nm in keep)
        r = reader_cls(io.BytesIO(stream))
        try:
            if kind.startswith("floor"):
                m = r.read_floor_ys(output_dim=dim, **kw)
            else:
                m = r.read_residue_ys(output_dim=dim, **kw)
            out["c%d" % i] = np.asarray(m, np.float32)
        except Exception as e:  # noqa: BLE001 — the reference's failure is part of the golden
            out["e%d" % i] = np.array("%s: %s" % (type(e).__name__, e))
    np.savez_compressed(os.path.join(GOLDEN, "features_%s.npz" % name), **out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("PARSEOGGVORBIS_REF", "/root/reference"))
    ap.add_argument("names", nargs="*")
    a = ap.parse_args()
    ours = os.path.join(ROOT, "oracle", "_ref", "ours.bin")
    assert os.path.exists(ours), "build oracle/_ref/ours.bin first (__graft_entry__.build())"
    reader_cls = load_reader_class(a.ref)
    for nm in a.names or FILES:
        o = make(nm, reader_cls, ours)
        print(nm, " ".join("%s:%s" % (k, o[k].shape if k.startswith("c") else "ERR") for k in sorted(o) if k != "grid"))


if __name__ == "__main__":
    main()
