"""The layout of vsyn_tuning_spec (include/vorbis_synth_hip.h, "tuning estimation") as the binding mirrors it, and the header's own
words for it."""
import ctypes as C
import os
import re

from parseoggvorbis_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tuning_spec_layout():
    T = binding.TuningSpec
    assert C.sizeof(T) == 40
    names = ("fmin", "fmax", "threshold", "resolution", "bins_per_octave", "reserved")
    assert [n for n, _ in T._fields_] == list(names)
    assert [getattr(T, n).offset for n in names] == [0, 8, 16, 24, 32, 36]
    assert [getattr(T, n).size for n in names] == [8, 8, 8, 8, 4, 4]
    assert (binding.VSYN_TUNING_ONLY, binding.VSYN_TUNING_ROWS) == (0, 1)


def test_the_header_declares_the_same_fields_in_the_same_order():
    txt = open(os.path.join(ROOT, "include", "vorbis_synth_hip.h")).read()
    body = re.search(r"typedef struct vsyn_tuning_spec \{(.*?)\} vsyn_tuning_spec;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(ctype, n.strip()) for n in names.split(",")]
    assert fields == [("double", "fmin"), ("double", "fmax"), ("double", "threshold"), ("double", "resolution"),
                      ("uint32_t", "bins_per_octave"), ("uint32_t", "reserved")]
    assert re.search(r"#define VSYN_TUNING_ONLY 0u", txt) and re.search(r"#define VSYN_TUNING_ROWS 1u", txt)
