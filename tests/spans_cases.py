"""Batches of ids for the token spans (hutk_spans.hip) placed by the kernels' own constants: a tile of SP_TILE ids, a
thread's SP_PER tokens, the wavefronts of a workgroup, the 64-byte blocks and 16 KiB chunks of the rank structure.  The
span entry points take ANY ids whose decodings tile the text, so no encoder is needed: a builder chooses the ids (and,
for an id of -1, the bytes of the one item it covers), the text is what decode_ref.DecodeRef decodes them to, and every
span is known.  Plain builders without a GPU and without the library: tests/test_spans_cases_cpu.py holds every case to
its claims and pins expected() against spans_ref.batch, tests/test_gpu_spans_edges.py runs all of them.

A case is Case(name, data uint8, offsets int64, ids int32, id_offsets int64, claims); claims says what the case is for
(see measure()), and the CPU test recomputes it from the arrays."""
import random
from collections import namedtuple

import numpy as np

import decode_cases as DC
import spans_ref as S

SP_TILE, SP_THREADS, SP_PER, WAVE = 2048, 256, 8, 64  # hutk_debug_span_tile_ids(); SP_THREADS * SP_PER == SP_TILE
BLOCK, SPAN_CHUNK_BYTES = 64, 16384                   # hutk_debug_span_chunk_bytes()
KINDS = ("byte", "char")
FAMILIES = ("size", "start_position", "dense_start", "empty_token", "entry_width", "rank_edge", "unknown")
SIZES = [1, 7, 8, 9, 2047, 2048, 2049, 4096, 65 * 2048 + 1, 129 * 2048 + 5]
DEPTHS = {1, 63, 64, 65, 128}  # whole start-free tiles in front of a token: one, two and three look-back windows
N_BYTES = [63, 64, 65, 16383, 16384, 16385, 32768]
UNKNOWN_ITEMS = ["#".encode(), "ß".encode(), "€".encode(), "😂".encode()]  # characters the character vocabulary lacks

Case = namedtuple("Case", "name data offsets ids id_offsets claims")


class RefText:
    """spans_ref.TokenText's shape over a DecodeRef: the bytes of an id at a document's front and anywhere else."""

    def __init__(self, ref):
        self.ref = ref
        self._first, self._rest = {}, {}

    def _get(self, memo, i, off, ln):
        if i not in memo:
            r = self.ref
            memo[i] = None if i < 0 or i >= r.n or r.bad[i] else bytes(r.blob[int(off[i]):int(off[i] + ln[i])])
        return memo[i]

    def first(self, i):
        return self._get(self._first, i, self.ref.soff, self.ref.slen)

    def rest(self, i):
        return self._get(self._rest, i, self.ref.off, self.ref.len)


# ---- from ids to a case ---------------------------------------------------------------------------------------------
def assemble(v, name, ids, id_offsets, unknown=None, claims=None):
    """The case of these ids: the text is DecodeRef's decoding of them; unknown {index: bytes} gives the item under every
    id of -1."""
    ids = np.asarray(ids, dtype=np.int32)
    oo = np.asarray(id_offsets, dtype=np.int64)
    unknown = unknown or {}
    assert set(np.nonzero(ids == -1)[0].tolist()) == set(unknown), name
    ln, src, _ = v.ref._layout(ids, oo)
    ln = np.array(ln, dtype=np.int64)
    known = ln.copy()
    for j, b in unknown.items():
        ln[j] = len(b)
    n = len(ids)
    pos = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(ln, out=pos[1:])
    data = np.zeros(int(pos[n]), dtype=np.uint8)
    tok = np.repeat(np.arange(n, dtype=np.int64), known)
    before = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(known, out=before[1:])
    within = np.arange(int(before[n]), dtype=np.int64) - before[tok]
    data[pos[tok] + within] = v.ref.blob[src[tok] + within]
    for j, b in unknown.items():
        data[int(pos[j]):int(pos[j + 1])] = np.frombuffer(b, dtype=np.uint8)
    return Case(name, data, pos[oo], ids, oo, claims or {})


def from_docs(v, name, docs, claims=None):
    """docs: lists of pieces, an id or the bytes of an unknown item (the id is -1 there)."""
    ids, unknown, cuts = [], {}, []
    for doc in docs:
        for p in doc:
            if isinstance(p, bytes):
                unknown[len(ids)] = p
                ids.append(-1)
            else:
                ids.append(int(p))
        cuts.append(len(ids))
    return assemble(v, name, ids, [0] + cuts, unknown, claims)


def from_pieces(v, name, pieces, cuts, claims=None):
    """one stream of pieces, cut into documents that end at the given indices (repeats: empty documents) and at the end"""
    flat = from_docs(v, name, [pieces], claims)
    _ids, oo = DC.cut(flat.ids, cuts)
    unknown = {j: p for j, p in enumerate(pieces) if isinstance(p, bytes)}
    return assemble(v, name, flat.ids, oo, unknown, claims)


def one_byte_ids(v):
    """ids of one-byte tokens that decode alike first and elsewhere (ASCII letters and digits)"""
    chars = "etaoinshrdlu0123456789"
    return [v.id[c.encode()] if v.is_byte else v.id[c] for c in chars]


class Cursor:
    """Pieces laid down with the byte position known: pad_to() fills with one-byte tokens up to a position."""

    def __init__(self, v, rng):
        self.v, self.rng, self.pieces, self.cuts, self.at = v, rng, [], [], 0
        self.ones = one_byte_ids(v)

    def put(self, p):
        first = not self.pieces or (self.cuts and self.cuts[-1] == len(self.pieces))
        r = self.v.ref
        self.at += len(p) if isinstance(p, bytes) else int((r.slen if first else r.len)[p])
        self.pieces.append(p)

    def ordinary_to(self, pos, slack=24):
        """ordinary tokens while at least `slack` bytes remain, then one-byte tokens: exactly `pos`"""
        while self.at + slack < pos:
            self.put(self.rng.randrange(self.v.n_base))
        self.pad_to(pos)

    def pad_to(self, pos):
        assert self.at <= pos, (self.at, pos)
        while self.at < pos:
            self.put(self.rng.choice(self.ones))

    def cut(self):
        self.cuts.append(len(self.pieces))

    def case(self, name, claims=None):
        return from_pieces(self.v, name, self.pieces, self.cuts, claims)


# ---- the reference, vectorised -------------------------------------------------------------------------------------
def token_lengths(v, c):
    """bytes under every id of a case whose ids tile its text: a known id's decoded length, an id of -1 the one item at
    its place (a byte, or the character whose length the lead byte gives, cut short at the document's end)"""
    ln = np.array(v.ref.lengths(c.ids, c.id_offsets), dtype=np.int64)
    unk = np.nonzero(c.ids == -1)[0]
    if len(unk):
        before = np.zeros(len(ln) + 1, dtype=np.int64)
        np.cumsum(ln, out=before[1:])
        doc = np.searchsorted(c.id_offsets, unk, side="right") - 1
        acc = 0
        for j, d in zip(unk.tolist(), doc.tolist()):
            at = int(c.offsets[0] + before[j]) + acc
            b, room = int(c.data[at]), int(c.offsets[d + 1]) - at
            n = 1 if v.is_byte or b < 0x80 else 2 if b & 0xE0 == 0xC0 else 3 if b & 0xF0 == 0xE0 else 4 if b & 0xF8 == 0xF0 else 1
            ln[j] = min(n, room)
            acc += int(ln[j])
    return ln


def expected(v, c, unit):
    """What spans_ref.batch gives for a case of status 0, with numpy: int64 [n_ids, 2].  (The CPU test holds the two
    equal on every family.)"""
    ln = token_lengths(v, c)
    n = len(ln)
    end = np.cumsum(ln) + int(c.offsets[0])
    start = end - ln
    doc = np.repeat(np.arange(len(c.offsets) - 1), np.diff(c.id_offsets))
    base = c.offsets[doc]
    out = np.zeros((n, 2), dtype=np.int64)
    if unit == "byte":
        out[:, 0], out[:, 1] = start - base, end - base
        return out
    cs = np.zeros(len(c.data) + 1, dtype=np.int64)
    np.cumsum((c.data & 0xC0) != 0x80, out=cs[1:])
    out[:, 0] = np.where(ln > 0, cs[np.minimum(start + 1, len(c.data))] - 1, cs[start]) - cs[base]
    out[:, 1] = cs[end] - cs[base]
    return out


# ---- what a case is for ----------------------------------------------------------------------------------------------
def start_class(i):
    """(tile, wavefront, lane, slot) of token i in k_sp_tiles"""
    r = i % SP_TILE
    return (i // SP_TILE, r // (WAVE * SP_PER), r // SP_PER % WAVE, r % SP_PER)


def measure(v, c):
    """From the arrays alone:
    starts        (tile, wavefront, lane, slot) of every token that starts a document
    empty_at      the same for every token (or the end of the ids) that empty documents sit on
    unknown_at    the same for every id of -1
    empty_run     the longest run of empty documents
    depths        for every tile whose first token starts no document: the whole start-free tiles in front of it
    tile_starts   the most document starts in one tile
    ends64 / ends16384 / bases64 / bases16384   residues of the token ends and of the bases of documents with ids
    cont_blocks   aligned 64-byte blocks of the text without a character start
    n_bytes, n_ids, n_docs"""
    oo, offs = c.id_offsets, c.offsets
    n_ids, n_docs = len(c.ids), len(offs) - 1
    has = oo[1:] > oo[:-1]
    first = oo[:-1][has]
    m = {"n_bytes": int(offs[-1]), "n_ids": n_ids, "n_docs": n_docs}
    m["starts"] = {start_class(int(i)) for i in first}
    m["empty_at"] = {start_class(int(i)) for i in oo[:-1][~has]}
    m["unknown_at"] = {start_class(int(i)) for i in np.nonzero(c.ids == -1)[0]}
    run = best = 0
    for h in has.tolist():
        run = 0 if h else run + 1
        best = max(best, run)
    m["empty_run"] = best
    n_tiles = (n_ids + SP_TILE - 1) // SP_TILE
    per_tile = np.bincount(first // SP_TILE, minlength=max(n_tiles, 1))
    m["tile_starts"] = int(per_tile.max()) if n_ids else 0
    is_first = np.zeros(n_ids + 1, dtype=bool)
    is_first[first] = True
    depths = set()
    for t in range(1, n_tiles):
        if not is_first[t * SP_TILE]:
            k = 0
            while per_tile[t - 1 - k] == 0:
                k += 1
            depths.add(k)
    m["depths"] = depths
    ends = np.cumsum(token_lengths(v, c)) + int(offs[0])
    bases = offs[:-1][has]
    for key, a in (("ends", ends), ("bases", bases)):
        for mod in (BLOCK, SPAN_CHUNK_BYTES):
            m["%s%d" % (key, mod)] = set((a % mod).tolist())
    whole = len(c.data) // BLOCK * BLOCK
    is_start = (c.data[:whole] & 0xC0) != 0x80
    m["cont_blocks"] = int((~is_start.reshape(-1, BLOCK).any(axis=1)).sum()) if whole else 0
    return m


def holds(claims, m):
    """Every claim against what measure() found: a set is contained, a number is reached, n_bytes is met exactly; `cont`
    lists byte positions that hold continuation bytes (checked by the caller against the data)."""
    for key, want in claims.items():
        if key == "cont":
            continue
        got = m[key]
        ok = want <= got if isinstance(want, (set, frozenset)) else got == want if key == "n_bytes" else got >= want
        if not ok:
            return "%s: claimed %r, measured %r" % (key, want, got if not isinstance(got, set) else sorted(got)[:40])
    return None


# ---- families --------------------------------------------------------------------------------------------------------
def size_cases(v, seed=21):
    """ONE document of n ordinary ids; the 129-tile batch has a document of SP_PER - 3 ids cut out of its front, so the long
    one starts inside a thread's tokens and its tokens see every look-back depth of DEPTHS."""
    rng = random.Random(seed)
    out = []
    for n in SIZES:
        ids = DC.ordinary(v, rng, n)
        last = (n - 1) // SP_TILE
        if n == SIZES[-1]:
            claims = {"depths": set(DEPTHS), "starts": {(0, 0, 0, 0), (0, 0, 0, 5)}, "n_ids": n}
            out.append(assemble(v, "n%d_cut_front" % n, *DC.cut(ids, [5]), claims=claims))
        else:
            claims = {"depths": {last - 1} if last >= 1 else set(), "starts": {(0, 0, 0, 0)}, "n_ids": n}
            out.append(assemble(v, "n%d_one_doc" % n, *DC.cut(ids, []), claims=claims))
    return out


START_TILES, START_LANES = (0, 1, 2), (0, 1, 63)


def start_positions():
    return sorted(t * SP_TILE + w * WAVE * SP_PER + l * SP_PER + k
                  for t in START_TILES for w in range(SP_THREADS // WAVE) for l in START_LANES for k in range(SP_PER))


def start_position_cases(v, seed=22):
    """About four tiles, a document start on every slot of lanes 0, 1 and 63 of every wavefront of tiles 0 .. 2: as cut,
    with an empty document on every such start, and with 300 empty documents at the front, on token 2047, on token 2048
    and at the end."""
    rng = random.Random(seed)
    n = 4 * SP_TILE + 37
    ids = DC.ordinary(v, rng, n)
    pos = start_positions()
    classes = {start_class(p) for p in pos}
    assert len(classes) == 3 * 4 * 3 * SP_PER
    out = [assemble(v, "starts_as_cut", *DC.cut(ids, pos[1:]), claims={"starts": classes})]
    out.append(assemble(v, "starts_with_an_empty_document_each", *DC.cut(ids, pos + pos),
                        claims={"starts": classes, "empty_at": classes}))
    runs = [0] * 300 + [SP_TILE - 1] * 300 + [SP_TILE] * 300 + [n] * 300
    at = {start_class(0), start_class(SP_TILE - 1), start_class(SP_TILE), start_class(n)}
    out.append(assemble(v, "starts_with_runs_of_300_empty_documents", *DC.cut(ids, pos[1:] + runs),
                        claims={"starts": classes, "empty_at": at, "empty_run": 300}))
    return out


def dense_start_cases(v, seed=23):
    """A tile that is all document starts, the same one token later, and documents of 0 .. 3 tokens over three tiles."""
    rng = random.Random(seed)
    ids = DC.ordinary(v, rng, SP_TILE + 701)
    out = [assemble(v, "2048_one_token_docs", *DC.cut(ids[1:], list(range(1, SP_TILE + 1)) + [SP_TILE + 200, SP_TILE + 450]),
                    claims={"tile_starts": SP_TILE, "n_docs": SP_TILE + 3})]
    out.append(assemble(v, "2049_one_token_docs", *DC.cut(ids, list(range(1, SP_TILE + 2)) + [SP_TILE + 201, SP_TILE + 451]),
                        claims={"tile_starts": SP_TILE, "n_docs": SP_TILE + 4, "starts": {(1, 0, 0, 0), (1, 0, 0, 1)}}))
    ids = DC.ordinary(v, rng, 3 * SP_TILE + 11)
    out.append(assemble(v, "docs_0_to_3", *DC.cut_random(ids, rng, 0, 3), claims={"tile_starts": 900, "empty_run": 2}))
    return out


def first_differs(v):
    """the ids whose decoding at a document's front is not their decoding elsewhere"""
    r = v.ref
    return [i for i in range(r.n) if not r.bad[i] and (r.slen[i] != r.len[i] or bytes(r.blob[r.soff[i]:r.soff[i] + r.slen[i]])
                                                      != bytes(r.blob[r.off[i]:r.off[i] + r.len[i]]))]


def empty_token_cases(v, seed=24):
    """Character vocabulary: the prefix alone is no text at a document's front and a space elsewhere."""
    assert not v.is_byte
    rng = random.Random(seed)
    P, P3, E = v.id["▁"], v.id["▁▁▁"], v.id["▁eeeee"]
    x, y = v.id["e"], v.id["漢"]
    small = [[P], [P, x], [P3], [P3, P], [E, x, E, y], [P, P], [x, P, y], [P], [P], [y, P3, E], [P]]
    out = [from_docs(v, "prefix_in_small_documents", small, claims={"n_docs": len(small)}),
           from_docs(v, "text_of_no_bytes", [[P]] * 5, claims={"n_bytes": 0, "n_ids": 5})]
    front = DC.ordinary(v, rng, SP_TILE - 40)
    docs = [front[:700], front[700:]] + [[P]] * 2100 + [DC.ordinary(v, rng, 60), [P], DC.ordinary(v, rng, 40)]
    run_at = {start_class(SP_TILE - 40), start_class(SP_TILE - 1), start_class(SP_TILE), start_class(2 * SP_TILE)}
    out.append(from_docs(v, "2100_documents_of_the_prefix_alone", docs, claims={"starts": run_at, "tile_starts": SP_TILE}))
    diff = first_differs(v)
    docs = [[d, d, x] for d in diff] + [[y, d] for d in diff] + [[d] for d in diff]
    out.append(from_docs(v, "ids_that_differ_first_and_elsewhere", docs, claims={"n_docs": 3 * len(diff)}))
    return out


def width_ids(v):
    """{decoded length: id} around the 7 bytes a decode-table entry holds inline, with multi-byte characters inside
    (byte vocabulary: where it has such a token), and a run token that lives in the blob"""
    r, out = v.ref, {}
    for L in (range(5, 11) if not v.is_byte else range(5, 9)):
        same = [i for i in range(v.n_base) if r.len[i] == L and r.slen[i] == L]
        multi = [i for i in same if (r.blob[r.off[i]:r.off[i] + L] >= 0x80).any()]
        assert same and (multi or v.is_byte), L
        out[L] = (multi or same)[0]
    if v.is_byte:
        out[13] = v.run(b"-", 13)
        out[26] = v.run("é".encode(), 13)
    return out


def entry_width_cases(v, seed=25):
    """Every width first in a document, later in one and as the batch's very last token (behind 40 ordinary ids, so both
    forms of sp_fetch run); batches whose whole text is 1, 7, 15, 16 and 17 bytes."""
    rng = random.Random(seed)
    w = width_ids(v)
    ones = one_byte_ids(v)
    out = []
    for L, i in sorted(w.items()):
        x, y = rng.choice(ones), rng.randrange(v.n_base)
        out.append(from_docs(v, "width%d_placed" % L, [DC.ordinary(v, rng, 40), [i, x, y], [x, i, y], [i], [y, x, i]]))
        out.append(from_docs(v, "width%d_alone" % L, [[i]], claims={"n_bytes": L}))
    for total in (1, 7, 15, 16, 17):
        parts, left = [], total
        while left:
            L = max(k for k in list(w) + [1] if k <= left)
            parts.append(w[L] if L > 1 else ones[0])
            left -= L
        docs = [parts[:1], parts[1:]] if len(parts) > 1 else [parts]
        out.append(from_docs(v, "text_of_%d_bytes" % total, docs, claims={"n_bytes": total}))
    return out


EDGES = [BLOCK, 2 * BLOCK, SPAN_CHUNK_BYTES, 2 * SPAN_CHUNK_BYTES]
NEAR = {0, 1, BLOCK - 1}, {0, 1, SPAN_CHUNK_BYTES - 1}


def rank_edge_cases(v, seed=26):
    """Token ends and document bases on the multiples of 64 and 16384 and one byte either side; a character that lies
    across each of them, on each of its bytes; texts of exactly the sizes where the number of blocks and chunks changes;
    byte mode: blocks without a character start, and a document that begins inside them."""
    rng = random.Random(seed)
    out = []
    c = Cursor(v, rng)
    for e in EDGES:
        for d in (-1, 0, 1):
            c.ordinary_to(e + d)
            c.cut()
    c.ordinary_to(2 * SPAN_CHUNK_BYTES + 300)
    both = {"ends64": NEAR[0], "bases64": NEAR[0], "ends16384": NEAR[1], "bases16384": NEAR[1]}
    out.append(c.case("ends_and_bases_on_the_edges", claims=both))
    for d in (-1, 0, 1):  # the second byte of the character on the edge + d
        c = Cursor(v, rng)
        for e in EDGES:
            c.ordinary_to(e + d - 1)
            if v.is_byte:
                c.put(v.id[b"\xc3"])
                c.put(v.id[b"\xa9"])
            else:
                c.put(v.id["漢"])
            if e == 2 * BLOCK:
                c.cut()
        c.ordinary_to(2 * SPAN_CHUNK_BYTES + 100)
        out.append(c.case("character_across_the_edges%+d" % d, claims={"cont": [e + d for e in EDGES]}))
    for total in N_BYTES:
        c = Cursor(v, rng)
        c.ordinary_to(total // 3)
        c.cut()
        c.ordinary_to(total)
        out.append(c.case("text_of_%d_bytes" % total, claims={"n_bytes": total, "ends64": {total % BLOCK},
                                                              "ends16384": {total % SPAN_CHUNK_BYTES}}))
    if v.is_byte:
        cont = v.id[b"\x80"]
        docs = [DC.ordinary(v, rng, 50), DC.ordinary(v, rng, 10) + [cont] * 120, [cont] * 80 + DC.ordinary(v, rng, 10),
                DC.ordinary(v, rng, 30)]
        out.append(from_docs(v, "200_continuation_bytes", docs, claims={"cont_blocks": 2}))
    return out


def unknown_cases(v, seed=27):
    """Ids of -1 on purpose.  Character mode: over characters of 1, 2, 3 and 4 bytes that the vocabulary lacks; byte mode:
    over ASCII, lead and continuation bytes.  First, last and alone in a document, on both sides of a tile edge inside a
    document and across documents, and 2100 of them in a row inside one document."""
    rng = random.Random(seed)
    items = [b"a", b"\xc3", b"\xa9", b"\x80"] if v.is_byte else UNKNOWN_ITEMS
    x = one_byte_ids(v)
    docs = [DC.ordinary(v, rng, 30)]
    for u in items:
        docs += [[u, x[0], x[1]], [x[2], x[3], u], [u], [u, u], [x[4], u, x[5]], items, items[::-1]]
    out = [from_docs(v, "unknown_items_placed", docs)]
    n = 2 * SP_TILE + 50
    edge = {(0, 3, 63, 7), (1, 0, 0, 0), (1, 3, 63, 7), (2, 0, 0, 0)}
    for name, cuts in (("inside_a_document", [9]), ("across_documents", [SP_TILE - 1, SP_TILE, 2 * SP_TILE])):
        for turn in range(len(items)):  # every item on every one of the four places
            pieces = DC.ordinary(v, rng, n)
            for k, at in enumerate((SP_TILE - 1, SP_TILE, 2 * SP_TILE - 1, 2 * SP_TILE)):
                pieces[at] = items[(k + turn) % len(items)]
            out.append(from_pieces(v, "unknown_on_a_tile_edge_%s_turn%d" % (name, turn), pieces, cuts, claims={"unknown_at": edge}))
    pieces = DC.ordinary(v, rng, 1000) + [items[k % len(items)] for k in range(2100)] + DC.ordinary(v, rng, 1200)
    out.append(from_pieces(v, "2100_unknown_items_in_a_row", pieces, [300], claims={"depths": {0}, "n_ids": 4300}))
    return out


def replacement(v, i, first):
    """a known id whose text at this place has another first byte and another length than id i's"""
    tt = RefText(v.ref)
    have = tt.first(i) if first else tt.rest(i)
    for j in range(300, v.n_base):
        t = tt.first(j) if first else tt.rest(j)
        if t and have and t[0] != have[0] and len(t) != len(have) and S.starts_before(t)[-1] != S.starts_before(have)[-1]:
            return j
    raise AssertionError("no replacement for id %d" % i)


def tamper_cases(v, seed=28):
    """-> [(case, victim document, tampered ids, the reference's status for them)]: a victim that ends on a tile edge,
    a victim that the tiles behind it look back through (the replacement has another length: what is carried past the
    victim is wrong for it and must not reach its neighbours), and a victim among 2048 one-token documents."""
    rng = random.Random(seed)
    tt = RefText(v.ref)
    out = []

    def add(case, victim, at):
        bad = case.ids.copy()
        bad[at] = replacement(v, int(case.ids[at]), at == int(case.id_offsets[victim]))
        _sp, st = S.batch(tt, case.data, case.offsets, bad, case.id_offsets, v.is_byte, "byte", np.int64)
        out.append((case, victim, bad, st))

    ids = DC.ordinary(v, rng, 2 * SP_TILE + 90)
    case = assemble(v, "victim_ends_on_a_tile_edge", *DC.cut(ids, [500, SP_TILE - 60, SP_TILE, SP_TILE + 70]))
    add(case, 2, SP_TILE - 1)
    ids = DC.ordinary(v, rng, 4 * SP_TILE + 300)
    case = assemble(v, "victim_is_looked_back_through", *DC.cut(ids, [60, 100, 3 * SP_TILE + 100, 3 * SP_TILE + 130]),
                    claims={"depths": {0, 1}})
    add(case, 2, 150)
    case = dense_start_cases(v)[0]
    add(case, 1000, 1000)
    return out


BUILDERS = {"size": size_cases, "start_position": start_position_cases, "dense_start": dense_start_cases,
            "empty_token": empty_token_cases, "entry_width": entry_width_cases, "rank_edge": rank_edge_cases,
            "unknown": unknown_cases}
_vocabs, _cases, _want = {}, {}, {}


def vocab(kind):
    if kind not in _vocabs:
        _vocabs[kind] = DC.Vocab(kind)
    return _vocabs[kind]


def applies(family, kind):
    return kind == "char" or family != "empty_token"


def cases(family, kind):
    """the family's cases under a vocabulary, built once per process, the family in front of their names"""
    if (family, kind) not in _cases:
        made = BUILDERS[family](vocab(kind)) if applies(family, kind) else []
        _cases[family, kind] = [c._replace(name="%s/%s" % (family, c.name)) for c in made]
    return _cases[family, kind]


def want(kind, case, unit):
    """expected() once per case and unit; read only"""
    key = (kind, case.name, unit)
    if key not in _want:
        _want[key] = expected(vocab(kind), case, unit)
        _want[key].setflags(write=False)
    return _want[key]
