"""Device views off the 16-byte boundary, and the batches that drive the element-by-element paths through their values:
what tests/test_gpu_views.py runs on the GPU and tests/test_views_cpu.py holds to its claims without one.

A GPU data loader that slices one large device buffer into batches hands the entry points views whose data_ptr() is
aligned to the element type and to nothing more.  shifted() and guarded() make such views inside allocations of the
test's own; the builders below make batches whose sizes, piece boundaries and chunk states put every lane of those paths
to work.  Nothing here touches the package under test except for the two torch helpers."""
import random

import numpy as np

import norm_ref as NR

GUARD_BYTE = 0xA5


# ---- views --------------------------------------------------------------------------------------------------------------
def shifted(t, k):
    """A copy of the device tensor `t` that starts `k` elements into a larger tensor of its own (the caching allocator
    hands that one out aligned to 512 bytes, so the view's data_ptr() is k elements off the boundary)."""
    import torch
    n = t.numel()
    buf = torch.zeros(k + n + 16, dtype=t.dtype, device=t.device)
    view = buf[k:k + n]
    view.copy_(t.reshape(-1))
    return view


def guarded(n, shift, dtype, guard, tail=64, device="cuda:0"):
    """-> (view, check): an output view of `n` elements with `shift` elements of `guard` in front of it and `tail` behind,
    all of one allocation; check(what) reads the buffer back once and asserts that both guard zones still hold `guard`."""
    import torch
    buf = torch.full((shift + n + tail,), guard, dtype=dtype, device=device)
    view = buf[shift:shift + n]

    def check(what=""):
        host = buf.cpu().numpy()
        assert (host[:shift] == guard).all(), "%s: written in front of the output" % (what,)
        assert (host[shift + n:] == guard).all(), "%s: written behind the output" % (what,)
    return view, check


# ---- normalisation ------------------------------------------------------------------------------------------------------
def hungarian(n_bytes):
    """at least n_bytes of precomposed Hungarian text: its own NFC form, and no byte at or above NFC's lead byte 0xCC"""
    words = ["árvíztűrő", "tükörfúrógép", "hogy", "a", "és", "őszi", "ÚJSÁG", "Győr", "szőlő", "fűző", "12", "-", "az", "üveg"]
    out, n, i = [], 0, 0
    while n < n_bytes:
        w = words[(i * 7 + i // 3) % len(words)]
        out.append(w)
        n += len(w.encode("utf-8")) + 1
        i += 1
    return " ".join(out)


def clean_docs(chunk):
    """three documents of Hungarian text, 5 chunks and more in all: every chunk is clean under NFC"""
    text = hungarian(5 * chunk)
    return [p.encode("utf-8") for p in (text[:700], text[700:9000], text[9000:])]


def py_spill(data, p, ds, de):
    """hutk_norm.h spill(): the bytes at p .. that continue a well-formed character begun before p inside [ds, de)"""
    if p >= de or (data[p] & 0xC0) != 0x80:
        return 0
    for j in (1, 2, 3):
        q = p - j
        if q < ds:
            return 0
        b0 = data[q]
        if (b0 & 0xC0) == 0x80:
            continue
        n = 1 if b0 < 0x80 else 0 if b0 < 0xC2 or b0 > 0xF4 else 2 if b0 < 0xE0 else 3 if b0 < 0xF0 else 4
        if n and q + n <= de:
            try:
                bytes(data[q:q + n]).decode("utf-8")
            except UnicodeDecodeError:
                n = 0
        else:
            n = 0
        return q + n - p if q + n > p else 0
    return 0


def edge_spill(data, offs, P):
    """hutk_norm.h edge_spill(): nothing spills over a document boundary or over either end of the text"""
    if P <= 0 or P >= len(data):
        return 0
    d = int(np.searchsorted(offs, P, side="left"))  # the first document that starts at or behind P
    if int(offs[d]) == P:
        return 0
    return py_spill(data, P, int(offs[d - 1]), int(offs[d]))


def chunk_states(data, offs, lead, chunk):
    """The kernel's own rule (the header comment of csrc/hutk_normalize.hip, k_norm_sizes): a chunk is CLEAN when no byte
    of it, and not the first byte of the character behind it, is at or above the form's first unstable lead byte.
    -> [(clean, spill at the chunk's front)] for every chunk"""
    data = bytes(data)
    arr = np.frombuffer(data, dtype=np.uint8)
    out = []
    for c0 in range(0, len(data), chunk):
        c1 = min(c0 + chunk, len(data))
        behind = c1 + edge_spill(data, offs, c1)
        dirty = bool((arr[c0:c1] >= lead).any()) or (behind < len(data) and data[behind] >= lead)
        out.append((not dirty, edge_spill(data, offs, c0)))
    return out


def _filler(pos):
    """printable ASCII that differs between any two positions a small multiple of 16 apart"""
    return 0x21 + (pos * 31 + pos // 97) % 94


# A character that straddles the edge between a dirty chunk and the clean one behind it may be any character at all, so
# that clean chunk can start with a spill of 0, 1, 2 or 3 bytes under every form (these three leave one byte in front of
# the edge; no form changes them).
STRADDLE_FROM_DIRTY = {1: "\u00f8", 2: "\u20ac", 3: "\U0001f600"}
# Between two CLEAN chunks the straddling character has its lead byte in a clean chunk, so the lead byte is below the
# form's (hutk_norm.h: edge_spill -> spill decodes a well-formed character only, and those start at 0xC2 or above):
#   NFC   lead 0xCC: two-byte characters with lead 0xC2..0xCB: a spill of 0 or 1 (U+00E9, C3 A9)
#   NFD   lead 0xC3: two-byte characters with lead 0xC2 only: a spill of 0 or 1 (U+00A9, C2 A9)
#   NFKC, NFKD lead 0xC2: no multi-byte character starts below 0xC2: a spill of 0 only
# Spills of 2 and 3 need a lead byte of 0xE0 or above, which is at or above every form's lead byte: unreachable between
# clean chunks under every form.
STRADDLE_CLEAN = {"NFC": "\u00e9", "NFD": "\u00a9", "NFKC": None, "NFKD": None}
CHANGING = {"NFC": ("e\u0301", -1), "NFKC": ("e\u0301", -1), "NFD": ("\u00e9", 1), "NFKD": ("\u00e9", 1)}  # (text, bytes it grows by)
LASTS = (1, 15, 16, 17, 40)


def clean_behind_dirty(form, delta, spill, last, chunk, many=False):
    """-> (documents, intended len(output) - len(input)).  Chunk 0 holds `delta` characters that change length by one
    byte under the form and is padded with ASCII to exactly `chunk` bytes; behind it come three clean chunks and a last
    chunk of `last` bytes, so every clean chunk is copied to an address whose residue mod 16 differs from its source's by
    `delta`.  spill > 0: a character of spill + 1 bytes straddles the edge behind chunk 0, and a two-byte character every
    edge between clean chunks where the form allows one (STRADDLE_CLEAN).  many: document boundaries inside the clean
    chunks -- on the byte after the first spill, in the middle of a chunk, on the byte after a clean chunk's spill,
    exactly at a chunk edge (that edge has no straddling character), an empty document, and inside the last chunk."""
    text, grow = CHANGING[form]
    n = 4 * chunk + last
    raw = bytearray(_filler(p) for p in range(n))
    at = 3
    for _ in range(delta):
        b = text.encode("utf-8")
        raw[at:at + len(b)] = b
        at += len(b) + 2
    assert at < chunk - 8
    clean_edges = [2 * chunk, 4 * chunk] if many else [2 * chunk, 3 * chunk, 4 * chunk]
    if spill:
        b = STRADDLE_FROM_DIRTY[spill].encode("utf-8")
        raw[chunk - 1:chunk - 1 + len(b)] = b
        if STRADDLE_CLEAN[form]:
            b = STRADDLE_CLEAN[form].encode("utf-8")
            for e in clean_edges:
                raw[e - 1:e + 1] = b
    raw = bytes(raw)
    assert len(raw) == n
    if not many:
        return [raw], grow * delta
    cuts = [chunk + spill, chunk + 1000, 2 * chunk + 1, 3 * chunk, 3 * chunk + 77, 3 * chunk + 77, 4 * chunk + (last + 1) // 2]
    cuts = sorted(c for c in cuts if c <= n)
    bounds = [0] + cuts + [n]
    return [raw[a:b] for a, b in zip(bounds[:-1], bounds[1:])], grow * delta


def clean_behind_dirty_cases(form):
    """every (delta, spill, last) the tests run for the form"""
    return [(m, sp, last) for m in range(1, 17) for sp in (0, 1, 2, 3) for last in LASTS]


# ---- token spans --------------------------------------------------------------------------------------------------------
SPAN_CHUNK_BYTES, SP_PER = 16384, 8


def spans_batch(orc):
    """-> (data uint8, offsets, ids int32, id offsets): documents of the C3 and C2 corpora, a little over two span
    chunks of text; an empty document first and last; short documents ("a", " b") in front of the last one until the
    total is no multiple of 16 and the number of ids (the oracle's, under its vocabulary) no multiple of SP_PER."""
    from hutoken_amd import synth
    docs = [b""]
    for corpus, n in (("C3", 400), ("C2", 40)):
        d, o = synth.corpus(corpus, n)
        raw = d.tobytes()
        docs += [raw[int(o[i]):int(o[i + 1])] for i in range(n)]
    body, size = [], 0
    for doc in docs:
        if size > 2 * SPAN_CHUNK_BYTES + 200:
            break
        body.append(doc)
        size += len(doc)
    last = next(doc for doc in docs[50:] if 10 < len(doc) < 400 and doc[-1] < 0x80)
    for k in range(64):
        batch = body + [b" b" if j % 3 else b"a" for j in range(k)] + [last, b""]
        data, offs = NR.pack(batch)
        ids, oo, st = orc.encode_packed(data, offs)
        if len(data) % 16 and len(ids) % SP_PER and not np.asarray(st).any():
            return data, offs, np.asarray(ids, dtype=np.int32), np.asarray(oo, dtype=np.int64)
    raise AssertionError("no padding of the span batch meets its size claims")


# ---- special tokens -----------------------------------------------------------------------------------------------------
CP_TILE = 2048
EOT = b"<|endoftext|>"
EOT_ID = 50256


def special_pieces(orc, docs, specials):
    """-> the output index at which every piece (text or marker, in order) of the batch begins, and the total"""
    import specials_ref as SR
    starts, total = [], 0
    for doc in docs:
        for p in SR.pieces(doc, specials):
            starts.append(total)
            total += len(orc.encode_bytes(p)[0]) if isinstance(p, bytes) else 1
    return starts, total


def special_batch(orc):
    """-> documents for the marker set {EOT: EOT_ID}: every document holds a marker; a text piece begins exactly at output
    id CP_TILE; the output is just over two CP_TILE long with a remainder that is no multiple of 4."""
    import helpers as H
    rng = random.Random(17)
    specials = {EOT: EOT_ID}

    def doc():
        t = H.random_text(rng, max_words=10).encode("utf-8")
        cut = rng.randint(0, len(t))
        while cut < len(t) and (t[cut] & 0xC0) == 0x80:
            cut += 1
        return t[:cut] + EOT + t[cut:] + (EOT if rng.random() < 0.3 else b"")

    docs = [EOT + b"x"]
    total = special_pieces(orc, docs, specials)[1]
    while True:  # random documents up to a little below CP_TILE ...
        d = doc()
        n = special_pieces(orc, [d], specials)[1]
        if total + n > CP_TILE - 1:
            break
        docs.append(d)
        total += n
    while total < CP_TILE - 1:  # ... documents of one marker each up to CP_TILE - 1 ...
        docs.append(EOT)
        total += 1
    docs.append(EOT + b" the piece behind this marker begins at the tile edge")  # ... the marker is id CP_TILE - 1
    total = special_pieces(orc, docs, specials)[1]
    while total <= 2 * CP_TILE + 8:
        d = doc()
        docs.append(d)
        total += special_pieces(orc, [d], specials)[1]
    while total % 4 == 0:
        docs.append(EOT)
        total += 1
    return docs


# ---- decode of byte-fallback ids ----------------------------------------------------------------------------------------
FBR_TILE = 1024
FB_TABLE_AT = (0, 3, 4, 1023, 1024)


def byte_table(entries):
    """the ids of the vocabulary's "<0xHH>" lines, as hutk_ctx_find_byte_tokens gives them"""
    by_key = {k: i for k, i in entries}
    return np.array([by_key[b"<0x%02X>" % b] for b in range(256)], dtype=np.int32)


def fallback_decode_batch(entries, table, special_ids=(), seed=23):
    """-> (ids int32[FBR_TILE + 1], id offsets): ids of the table at FB_TABLE_AT -- the first group of four, the next one
    and both sides of the pass's tile edge -- and ordinary tokens (and the special ids, where given) everywhere else; document
    boundaries inside a group of four, at the tile edge and an empty document."""
    rng = random.Random(seed)
    in_table = set(int(t) for t in table)
    pool = [i for _k, i in entries if i not in in_table] + list(special_ids) * 10
    ids = [rng.choice(pool) for _ in range(FBR_TILE + 1)]
    for k, at in enumerate(FB_TABLE_AT):
        ids[at] = int(table[(0xC3, 0xA9, 0x61, 0xF0, 0x9F)[k]])
    offs = np.array([0, 0, 2, 5, 700, FBR_TILE, FBR_TILE, FBR_TILE + 1], dtype=np.int64)
    return np.array(ids, dtype=np.int32), offs


# ---- collation ----------------------------------------------------------------------------------------------------------
COLLATE_L = 64


def collate_batch(seed=5, n_docs=300):
    """-> (ids int32, offsets): documents of 0 to 40 ids, negative ids among them"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 41, size=n_docs)
    offs = np.zeros(n_docs + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return rng.integers(-3, 60000, size=int(offs[-1])).astype(np.int32), offs
