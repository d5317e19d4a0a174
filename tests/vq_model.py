"""Residue decode from classifications and entry numbers, written from the Vorbis I specification, sections 8.6.2 - 8.6.5, in numpy:
an independent model of what the residue VQ stage computes (the bit reading of 8.6.2 is the host's half and is not modelled: the
classification per partition and the entry number per vector are the inputs).

  8.6.2  limit begin / end to the vector length; partitions_to_read = (end - begin) / partition_size; eight passes over the
         partitions; within a pass the vectors of the submap are visited partition by partition (ONE partition counter for all of
         them); a vector marked 'do not decode' is skipped; a class without a book in the pass reads nothing.
  8.6.3  format 0: entry k of a partition's `step = partition_size / dimensions` entries adds its component l to element
         offset + k + l * step.
  8.6.4  format 1: the entries' value vectors are added back to back from offset on.
  8.6.5  format 2: the submap's ch vectors are ONE interleaved vector of ch * n elements decoded as format 1 - always, unless every
         channel is marked 'do not decode', which the caller decides -, then element i * ch + j goes to element i of vector j.

Arithmetic: float32, one addition per element and pass, in pass order, onto vectors that start at +0 - the sums are the same bits on
any IEEE machine. Elements outside [begin, begin + partitions * partition_size) are never touched and stay zero.

No code is shared with oracle/ (tests/test_vq_model_cpu.py pins the two against each other)."""
import numpy as np


class BadStream(ValueError):
    pass


def _decode_vectors(vq_spec, r, fmt, nvec, decode, length, cls, entries, epos):
    """8.6.2 for nvec vectors of `length` elements -> (float32 [nvec][length], classifications consumed, new entry position).
    cls: uint8 [nvec * parts], vector-major (vector j's partitions at j * parts ...), as the stage's input lays them out."""
    out = np.zeros((nvec, length), np.float32)
    psize = int(r["partition_size"])
    begin = min(int(r["begin"]), length)
    end = min(int(r["end"]), length)
    if end <= begin:
        return out, 0, epos
    parts = (end - begin) // psize
    if cls.size < nvec * parts:
        raise BadStream("classifications run out")
    books = np.asarray(r["books"]).reshape(-1, 8)
    nclass = int(r["num_classifications"])
    for ps in range(8):
        for pc in range(parts):
            off = begin + pc * psize
            for j in range(nvec):
                if not decode[j]:
                    continue
                c = int(cls[j * parts + pc])
                if c >= nclass:
                    raise BadStream("classification out of range")
                b = int(books[c, ps])
                if b < 0:
                    continue
                dims, nent, tab = vq_spec.codebooks[b]
                if tab is None:
                    raise BadStream("book without values")
                step = psize // dims
                if epos + step > entries.size:
                    raise BadStream("entries run out")
                e = entries[epos:epos + step].astype(np.int64)
                epos += step
                if (e >= nent).any():
                    raise BadStream("entry number out of range")
                vals = np.asarray(tab, np.float32).reshape(nent, dims)[e]  # [step][dims]
                # format 0: element k + l * step <- component l of entry k; format 1: element k * dims + l
                add = vals.T.reshape(-1) if fmt == 0 else vals.reshape(-1)
                seg = out[j, off:off + psize]
                np.add(seg, add, out=seg)  # float32 + float32, one rounding
    return out, nvec * parts, epos


def residue_vq(vq_spec, mapping, channels, n2, used_mask, cls, entries):
    """One packet -> float32 [channels * n2] (channel-major), the vectors after residue decode and before coupling.
    used_mask: bit c set = channel c is decoded (the floor 'unused' flags after the coupling step has propagated them).
    Raises BadStream where the numbers do not describe a packet of this setup (including entries left over)."""
    mux, sres = vq_spec.mappings[mapping]
    cls = np.asarray(cls, np.uint8)
    entries = np.asarray(entries, np.uint16)
    out = np.zeros((channels, n2), np.float32)
    cpos = epos = 0
    for s in range(len(sres)):
        chans = [c for c in range(channels) if mux[c] == s]
        if not chans:
            continue
        r = vq_spec.residues[sres[s]]
        ch = len(chans)
        if int(r["type"]) == 2:
            v, used, epos = _decode_vectors(vq_spec, r, 1, 1, [True], ch * n2, cls[cpos:], entries, epos)
            out[chans, :] = v[0].reshape(n2, ch).T
        else:
            decode = [bool((used_mask >> c) & 1) for c in chans]
            v, used, epos = _decode_vectors(vq_spec, r, int(r["type"]), ch, decode, n2, cls[cpos:], entries, epos)
            out[chans, :] = v
        cpos += used
    if epos != entries.size:
        raise BadStream("entries left over")
    return out.reshape(-1)
