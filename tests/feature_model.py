"""Independent numpy model of the feature matrices (include/vorbis_synth_hip.h, "feature matrices"), written from the stated semantics
and fed by the CPU oracle's taps (unwrapped posts `floor_final`, rendered curve `floor_curve`) on a batch: what the GPU tests compare
vsyn_features_host against, and what tests/test_features_cpu.py pins to the reference's own matrices (tests/golden/features_*.npz).

model_features(spec, batch, kind, output_dim, **kwargs) -> list of per-segment float32 matrices, or ModelError where the reference
raises (reason "index": an xs index past the floor vector; "broadcast": floor_base and row lengths differ; "assert": output_dim below
the biggest floor's post count for a residue kind without ignore_xs)."""
import math

import numpy as np

from oracle import oracle_binding as ob

F32 = np.float32


class ModelError(Exception):
    def __init__(self, reason, msg=""):
        super().__init__("%s: %s" % (reason, msg))
        self.reason = reason


def zoom_round(xs, z):
    """scipy.ndimage.zoom(float32 xs, z, order=1, mode='nearest') then numpy.round -> int list, or None where the output length is
    not len(xs) * z (the reference asserts)."""
    L = len(xs)
    want = L * z
    outn = round(want)
    if outn != want:
        return None
    zf = (L - 1) / (outn - 1) if outn > 1 else 1.0
    x = [float(np.float32(v)) for v in xs]
    out = []
    for k in range(outn):
        cc = min(max(k * zf, 0.0), L - 1.0)
        s = math.floor(cc)
        t = cc - s
        v = 0.0 + (1.0 - t) * x[s]
        v = v + t * x[min(s + 1, L - 1)]
        out.append(int(np.round(np.float32(v))))
    return out


def _taps(spec, b):
    P = len(b["packets"])
    streams = int(b["segments"]["stream"].max()) + 1 if len(b["segments"]) else 1
    plane = b.get("plane_stride") or (P * spec.blocksize1 // 2 + 64)
    r = ob.OracleSynth(spec, max_streams=max(streams, 1)).submit_host(b["packets"], b["segments"], b["ys"], b["residue"], plane,
                                                                     want_taps=True)
    assert r["rc"] == 0, ("oracle refused the batch", r["flags"])
    return r["taps"]


class _Curve:
    """The floor vector of one (packet, channel) row: n entries, the oracle's curve tap for x < n/2, above that the closed form
    over the flagged sorted posts (flat after the last)."""

    def __init__(self, xs, row, tap):
        self.xs, self.row, self.tap = xs, row, tap
        order = sorted(range(len(xs)), key=lambda i: xs[i])
        self.pts = [(xs[i], int(row[i]) & 0x7FFF) for i in order if (int(row[i]) >> 15) or i == 0]

    def at(self, x):
        if x < len(self.tap):
            return int(self.tap[x])
        lx, ly = self.pts[0]
        for hx, hy in self.pts[1:]:
            if x < hx:
                dy = hy - ly
                off = (abs(dy) * (x - lx)) // (hx - lx)
                return ly + off if dy >= 0 else ly - off
            lx, ly = hx, hy
        return ly


def _to_float(v, positive):
    v = np.asarray(v, F32)
    return v / F32(255.0) if positive else (v - F32(127.5)) / F32(127.5)


def model_features(spec, b, kind, output_dim, taps=None, **kw):
    C, D = spec.channels, int(output_dim)
    taps = taps if taps is not None else _taps(spec, b)
    pk, seg = b["packets"], b["segments"]
    P = len(pk)
    stride = spec.ys_stride
    ff = taps["floor_final"].reshape(P, C, stride)
    curve = taps["floor_curve"]
    Fn = len(spec.floors)
    posts = [len(xs) for _, xs in spec.floors]
    big = max(range(Fn), key=lambda f: posts[f])  # the first of the largest
    xs = [sorted(x) if kw.get("sorted_xs") else list(x) for _, x in spec.floors]
    floor_kind = kind.startswith("floor")
    up = xs
    if floor_kind and kw.get("upscale_xs_factor", 1) != 1:
        up = [zoom_round(x, kw["upscale_xs_factor"]) for x in xs]
        if any(u is None for u in up):
            raise ModelError("assert", "upscale length")
    include = kw.get("include_floor_number", None)
    only_big = kw.get("only_biggest_floor", False)
    if only_big:
        include = False
    include = include is None or bool(include)
    o = 1 if (floor_kind and include) else 0
    ignore = kw.get("ignore_xs", False)
    if not floor_kind and not ignore and D < posts[big]:
        raise ModelError("assert", "output_dim below the biggest floor's posts")
    out = []
    for g in seg:
        rows = []
        off = int(g["residue_off"])
        floor_base = None
        for p in range(int(g["first_packet"]), int(g["first_packet"]) + int(g["num_packets"])):
            mode = int(pk[p]["mode"])
            lng, mapping = spec.modes[mode]
            n = spec.blocksize1 if lng else spec.blocksize0
            chf = spec.mappings[mapping][1]
            used = int(pk[p]["floor_used"])

            def crv(c):
                return _Curve(list(spec.floors[chf[c]][1]), ff[p, c], curve[off + c * (n // 2): off + (c + 1) * (n // 2)])

            for c in range(C):
                if not (used >> c) & 1:
                    continue
                f = chf[c]
                if floor_kind:
                    if only_big and f != big:
                        continue
                    row = np.zeros(D, F32)
                    if o:
                        row[0] = (f + 1.0) / Fn - 0.5
                    if kind == "floor_final_ys":
                        vals = [int(ff[p, c, j]) & 0x7FFF for j in range(posts[f])][:D - o]
                    else:
                        if kw.get("xs_from_biggest_floor"):
                            lst = np.array(up[big], np.int64)
                            if f != big:
                                factor = int(round(float(max(xs[big])) / float(max(xs[f]))))
                                lst = lst // factor if factor else np.zeros_like(lst)
                            lst = np.clip(lst, 0, n - 1)
                        else:
                            lst = np.array(up[f], np.int64)
                            if lst.max() >= n:
                                raise ModelError("index", "packet %d channel %d: index %d, vector of %d" % (p, c, lst.max(), n))
                        cv = crv(c)
                        vals = [cv.at(int(x)) for x in lst[:max(0, D - o)]]
                    fl = _to_float(vals, kw.get("floor_always_positive", False))
                    row[o:o + len(fl)] = fl
                    rows.append(row)
                elif kind == "residue_ys_with_floor" and f == big:
                    idx = np.arange(min(n, D)) if ignore else np.clip(np.array(xs[big][:D], np.int64), 0, n - 1)
                    cv = crv(c)
                    floor_base = np.array([cv.at(int(x)) for x in idx], F32) / F32(255.0)
            if floor_kind or chf[C - 1] != big:
                off += C * (n // 2)
                continue
            n2 = n // 2
            idx = np.arange(min(n2, D)) if ignore else np.clip(np.array(xs[big][:D], np.int64), 0, n2 - 1)
            for c in range(C):
                sel = np.array(b["residue"][off + c * n2: off + (c + 1) * n2], F32)[idx]
                if kw.get("log1p_abs_space"):
                    sel = np.log1p(np.abs(sel))
                if floor_base is not None:
                    if len(floor_base) != len(sel) and 1 not in (len(floor_base), len(sel)):
                        raise ModelError("broadcast", "floor_base %d vs row %d" % (len(floor_base), len(sel)))
                    fbf = kw.get("floor_base_factor", 1)
                    if kw.get("log1p_abs_space"):
                        sel = sel + floor_base * F32(fbf)
                    else:
                        sel = sel * np.exp((floor_base - F32(1.0)) * F32(fbf))
                scale = kw.get("scale", 1.0)
                if scale != 1:
                    sel = sel * F32(scale)
                cl = kw.get("clip_abs_max", None)
                if cl is not None and cl > 0:
                    sel = np.clip(sel, F32(-cl), F32(cl))
                row = np.zeros(D, F32)
                row[:len(sel)] = sel
                rows.append(row)
            off += C * n2
        out.append(np.array(rows, F32).reshape(len(rows), D))
    return out


def spec_from_synth_npz(z):
    """The SetupSpec of a tests/golden/synth_*.npz / winflags_*.npz stream (the setup oracle/make_synth_ogg.py wrote)."""
    from parseoggvorbis_amd.binding import SetupSpec
    C = int(z["channels"])
    floors = [(int(z["floor%d_mult" % f]), [int(v) for v in z["floor%d_xs" % f]]) for f in range(int(z["num_floors"]))]
    maps = []
    m = 0
    while "chfloor_m%d" % m in z.files:
        maps.append(([(int(a), int(b)) for a, b in z["coupling_m%d" % m]], [int(v) for v in z["chfloor_m%d" % m]]))
        m += 1
    modes = [(int(bf), int(mp)) for bf, mp in zip(z["mode_blockflag"], z["mode_mapping"])]
    return SetupSpec(C, int(z["blocksize0"]), int(z["blocksize1"]), floors, maps, modes)
