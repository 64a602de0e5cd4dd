"""Decoding ids with special ids among them, restated from the contract of include/hutoken_amd.h in plain Python on top of
tests/decode_ref.py (own code).

`specials` is what was installed, in order: a list of (bytes, id) pairs (or a dict {bytes: id}).  An id is special when
a pair has it; its string is that of the FIRST such pair.

    flags 0   the special ids cut a document into runs of ordinary ids; every run is decoded as a document of its own
              (DecodeRef.decode_doc / decode_packed: one prefix comes off its front), every special gives its string
    skip      the special ids are deleted, what is left is decoded as one document

decode_doc() does that a document at a time, by the definition.  decode_packed() and status() do it for a batch by
refining the offsets -- every run a document -- and calling DecodeRef.decode_packed / status on them; the two forms are
compared in tests/test_decode_special_cpu.py, the GPU in tests/test_gpu_decode_special.py with the packed one."""
import numpy as np


def strings(specials):
    """{id: bytes}: the string of every special id (the first pair that carries it)"""
    pairs = specials.items() if isinstance(specials, dict) else specials
    out = {}
    for s, i in pairs:
        out.setdefault(int(i), bytes(s))
    return out


def decode_doc(ref, ids, specials, skip=False):
    """One document by the definition -> (bytes, status); a bad ordinary id: (b"", its code), as DecodeRef.decode_doc."""
    text = strings(specials)
    if skip:
        return ref.decode_doc([int(i) for i in ids if int(i) not in text])
    out, run = bytearray(), []
    for i in list(ids) + [None]:
        if i is None or int(i) in text:
            piece, st = ref.decode_doc(run)
            if st:
                return b"", st
            out += piece
            run = []
            if i is not None:
                out += text[int(i)]
        else:
            run.append(int(i))
    return bytes(out), 0


def _refine(ids, id_offsets, text):
    """-> (is_special bool[n], ordinary ids, offsets of the runs over the ordinary ids, run index of every document's
    first run [n_docs + 1]).  Document d's runs are first[d] .. first[d + 1] - 1: one more than it has specials."""
    ids = np.asarray(ids, dtype=np.int64)
    offs = np.asarray(id_offsets, dtype=np.int64)
    sp = np.isin(ids, np.fromiter(text.keys(), dtype=np.int64, count=len(text))) if len(text) else np.zeros(len(ids), bool)
    before = np.concatenate([[0], np.cumsum(sp)])  # specials in ids[0, i)
    first = np.arange(len(offs), dtype=np.int64) + before[offs]
    n_runs = (len(offs) - 1) + int(before[-1])
    # a run ends at every special and at every document end; positions counted in ORDINARY ids
    ordinary_before = np.arange(len(ids) + 1, dtype=np.int64) - before
    ends = np.empty(n_runs, dtype=np.int64)
    where_sp = np.nonzero(sp)[0]
    # the special at position p of document d closes run (d + specials before p)
    doc_of = np.searchsorted(offs, where_sp, side="right") - 1
    ends[doc_of + before[where_sp]] = ordinary_before[where_sp]
    ends[first[1:] - 1] = ordinary_before[offs[1:]]
    run_offs = np.concatenate([[0], ends])
    return sp, ids[~sp], run_offs, first


def decode_packed(ref, ids, id_offsets, specials, skip=False):
    """-> (bytes uint8, out_offsets int64[n_docs + 1]).  A bad id contributes no bytes, as in DecodeRef.decode_packed."""
    text = strings(specials)
    offs = np.asarray(id_offsets, dtype=np.int64)
    sp, ordinary, run_offs, first = _refine(ids, offs, text)
    if skip:
        before = np.concatenate([[0], np.cumsum(sp)])
        return ref.decode_packed(ordinary, offs - before[offs])
    raw, run_oo = ref.decode_packed(ordinary, run_offs)
    raw = raw.tobytes()
    ids = np.asarray(ids, dtype=np.int64)
    parts, oo, total, run = [], np.zeros(len(offs), dtype=np.int64), 0, 0
    for d in range(len(offs) - 1):
        for p in range(int(offs[d]), int(offs[d + 1]) + 1):  # (the document's end closes its last run)
            if p == offs[d + 1] or sp[p]:
                piece = raw[int(run_oo[run]):int(run_oo[run + 1])]
                run += 1
                parts.append(piece)
                total += len(piece)
                if p < offs[d + 1]:
                    parts.append(text[int(ids[p])])
                    total += len(parts[-1])
        oo[d + 1] = total
    assert run == len(run_offs) - 1 == first[-1]
    return np.frombuffer(b"".join(parts), dtype=np.uint8), oo


def status(ref, ids, id_offsets, specials):
    """int32[n_docs]: the code of a document's bad ORDINARY id (a special id is never bad), either flag."""
    text = strings(specials)
    offs = np.asarray(id_offsets, dtype=np.int64)
    sp, ordinary, _run_offs, _first = _refine(ids, offs, text)
    before = np.concatenate([[0], np.cumsum(sp)])
    return ref.status(ordinary, offs - before[offs])
