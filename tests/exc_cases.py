"""Vocabulary kinds and long-word inputs of tests/test_gpu_exc_kinds.py (checked without a GPU by tests/test_exc_cases_cpu.py),
seeded.

Which routine encodes an exception word (more than 32 units or 63 bytes, an end its tile cannot see, items of several
units) depends on the tables' kind, on the tail the host enqueues and on the word's length.  Here: one small generated
vocabulary per kind (KINDS), words glued from the kind's own multi-character keys (random letters hardly merge) with their
length in UNITS on every limit of the routines (LIMITS), each in every position (FORMS), and three batch shapes: all
documents at once (the full tail), consecutive batches of 5..32 tiles (k_tail_small), and batches of at most four tiles
(the one-launch k_tiles of the host form).

The restatements below are plain Python: the words as the tile kernel sees them (the reference's splitter plus the seam
map's cuts), the units of a word (bytes or characters, plus the expansion of items of several units, plus the prefix), and
the list a word goes on (exc_list_of in csrc/hutk_exc.h, d_exc_lane / d_exc_medium / k_tiles for the words up to 63 bytes)."""
import random
from collections import namedtuple

import helpers as H
from hutoken_amd import vocab_files as vf

TILE = 960
SMALL_TILES, SMALL_DOCS, ONE_TILES = 32, 4096, 4
LANE_MAX_UNITS, LANE_MAX_BYTES, MEDIUM_UNITS = 32, 63, 64
# a word's length in units, the prefix counted where the word gets one: the limits of d_exc_lane / d_exc_medium (32 units,
# 63 bytes, 64 units), of the four lists (128, 256, 512, 1024), of d_exc's LDS forms (1024 and 2046 units) and beyond
LIMITS = [31, 32, 33, 62, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2045, 2046, 2047,
          2048, 2049, 3000]
GIANT = (65536, 65537)  # bpe_wave_big's chunk size steps from 64 to 128 units between the two
FORMS = ("alone", "space-first", "behind-short", "short-behind", "long-behind")
ONE_LAUNCH_MAX = 3800

# tag -> (byte mode, prefix, 32-bit symbols, rank == symbol order, items of several units, merges file)
KINDS = {
    "B16":   (True, None, False, True, False, False),
    "B16d":  (True, None, False, False, False, False),
    "C16s":  (False, "▁", False, False, False, False),
    "B32":   (True, None, True, True, False, False),
    "B32s":  (True, None, True, False, False, False),
    "C32":   (False, "▁", True, True, False, False),
    "C32s":  (False, "▁", True, False, False, False),
    "B32m":  (True, None, True, True, False, True),
    "B16x":  (True, None, False, True, True, False),
    "B16xm": (True, None, False, True, True, True),
    "C16xm": (False, "▁", False, True, True, True),
    "B32x":  (True, None, True, True, True, False),
    "P2":    (False, "▁▁", False, True, False, False),
}
GIANT_KINDS = ("B16d", "B32s", "C32s", "B16x")
ONE_LAUNCH_KINDS = tuple(k for k, v in KINDS.items() if not v[4])  # one_shot_takes refuses items of several units
N_32 = 70000  # merges of the 32-bit kinds (more than 65520 symbols)

Kind = namedtuple("Kind", "tag vp sp mp prefix is_byte sym32 rank_is_sym multi merges n_prefix scale pieces seams")

LETTERS_1 = "etaoinshrdlucmfwypvbgkqjxz"
LETTERS_2 = H.HU
LETTERS_3 = H.CJK[:6]


def fast_char_vocab(seed, n_merges, max_len=24, special=None):
    """random_char_vocab's shape (byte-fallback literals, single characters, merges of earlier tokens) built as
    random_byte_vocab builds its own: the left half is an earlier token or one character, the right half an earlier token,
    and keys may be up to max_len characters -- 70 000 merges in a second or two, where max_len=10 rejects most candidates."""
    rng = random.Random(seed)
    chars = list("▁" + LETTERS_1 + "ETAOIN0123456789.,!?-") + list(LETTERS_2) + list(LETTERS_3)
    toks = ["<0x%02X>" % b for b in range(256)] + chars
    seen = set(toks)
    cjk = list(LETTERS_3)
    while len(toks) < 256 + len(chars) + n_merges:
        if all(c in LETTERS_3 for c in toks[-1]) and toks[-1] not in cjk:
            cjk.append(toks[-1])
        if rng.random() < 0.1:  # keys of three-byte characters only: the splitter makes words of their runs
            a, b = rng.choice(cjk), rng.choice(cjk)
        else:
            a = rng.choice(chars) if rng.random() < 0.35 else toks[rng.randrange(256, len(toks))]
            b = toks[rng.randrange(256, len(toks))]
        tok = a + b
        if tok in seen or len(tok) > max_len:
            continue
        seen.add(tok)
        toks.append(tok)
    entries = [(tk.encode("utf-8"), i) for i, tk in enumerate(toks)]
    return entries, (special if special is not None else {32: "▁"})


def shuffled_ids(entries, seed, first):
    """The ids of entries[first:] permuted among themselves, and one in ten of them given the id of another: the loader
    numbers symbols by id, so only keys that SHARE an id make rank and symbol order differ (Tables::rank_is_sym == 0)."""
    rng = random.Random(seed)
    ids = [i for _k, i in entries[first:]]
    rng.shuffle(ids)
    for _ in range(len(ids) // 10):
        ids[rng.randrange(len(ids))] = ids[rng.randrange(len(ids))]
    return entries[:first] + [(k, i) for (k, _i), i in zip(entries[first:], ids)]


def ordered_merges_text(entries, raw):
    """A merges file whose ranks rise with the ids: one rule per token that splits into two tokens, in id order."""
    keys = {r: k for r, (k, _i) in zip(raw, entries)}
    lines = ["#version: 0.2"]
    for r, (k, _i) in zip(raw, entries):
        if len(r) < 2 or b" " in r or b"\n" in r or b"\t" in r:
            continue
        for cut in range(len(r) - 1, 0, -1):
            a, b = r[:cut], r[cut:]
            if a in keys and b in keys:
                lines.append(keys[a].decode("utf-8") + " " + keys[b].decode("utf-8"))
                break
    return "\n".join(lines) + "\n"


def _raw_byte_tokens(entries):
    t = vf.bytes_to_unicode()
    back = {c: b for b, c in t.items()}
    return [bytes(back[c] for c in key.decode("utf-8")) for key, _i in entries]


def _letter_pieces(raws, letters, max_units):
    """The multi-character keys that are letters only (a word glued from them stays one word), as raw bytes."""
    ok = set(letters)
    out = []
    for r in raws:
        try:
            s = r.decode("utf-8")
        except UnicodeDecodeError:
            continue
        if 2 <= len(s) <= max_units and all(c in ok for c in s):
            out.append(s)
    return sorted(set(out))


_kinds = {}
_docs = {}


def kind(tag, tmpdir):
    """-> Kind: the vocabulary's files (written once per process under tmpdir), what the tables should say of it, the units
    an input byte expands to (scale: {byte: units}, 1 where absent) and the keys its words are glued from."""
    if tag in _kinds:
        return _kinds[tag]
    is_byte, prefix, sym32, rank_is_sym, multi, merges = KINDS[tag]
    n = N_32 if sym32 else 3000
    seed = 60 + sorted(KINDS).index(tag)
    if is_byte:
        ents, special = H.random_byte_vocab(seed, n, proper=True, dup_ids=(tag == "B16d"), max_len=16)
        raws = _raw_byte_tokens(ents)
        if tag == "B32s":
            ents = shuffled_ids(ents, seed, 256)
        pieces = {"1": _letter_pieces(raws[256:], LETTERS_1.replace("q", "") if multi else LETTERS_1, 16)}
    else:
        special = vf.llama_special_mapping() if multi else {32: "▁"}
        ents, special = fast_char_vocab(seed, n, special=special)
        raws = [k for k, _i in ents]
        if tag in ("C16s", "C32s"):
            first = next(i for i, (k, _i) in enumerate(ents) if len(k.decode("utf-8")) > 1 and not k.startswith(b"<0x"))
            ents = shuffled_ids(ents, seed, first)
        l1 = LETTERS_1.replace("q", "") if multi else LETTERS_1
        pieces = {"1": _letter_pieces(raws[256:], l1, 24), "12": _letter_pieces(raws[256:], l1 + LETTERS_2, 24),
                  "3": _letter_pieces(raws[256:], LETTERS_3, 24)}
    if multi:  # q -> "Alpha": five units inside a word of letters; the Llama file's "<0x09>": six units, a word each
        special = dict(special)
        special[ord("q")] = "Alpha"
    scale = {b: len(v) for b, v in special.items() if len(v) > 1} if multi else {}
    vp, sp = H.write_vocab(tmpdir, tag, ents, special)
    mp = None
    if merges:
        text = ordered_merges_text(ents, raws) if tag == "B32m" else H.random_merges_text(ents, seed, noise=False)
        mp = H.write_merges(tmpdir, tag, text)
    n_prefix = len(prefix) if prefix else 0
    k = Kind(tag, vp, sp, mp, prefix, is_byte, sym32, rank_is_sym, multi, merges, n_prefix, scale, pieces, None)
    ctx = host_context(k)
    _kinds[tag] = k._replace(seams=seams_of(ctx))
    ctx.close()
    return _kinds[tag]


def host_context(k):
    """Tables only (device = -2): table_stats, ids_capacity and the seam map without a GPU."""
    from hutoken_amd import _capi
    return _capi.Context(k.vp, k.sp, k.prefix, k.is_byte, device=-2, merges_path=k.mp)


def oracle(k, oracle_mod):
    return oracle_mod.Oracle(k.vp, k.sp, k.prefix, k.is_byte, merges_path=k.mp)


# ---- restatements ------------------------------------------------------------------------------------------

def seams_of(ctx):
    """-> the seam map as a list of 256 ints, or None when the context does not split by it."""
    m, on = ctx.seam_map()
    return [int(x) for x in m] if on else None


def gpu_words(doc, seams, split_words):
    """[(start, end)] of the words k_tiles makes of one document: the reference's word starts (split_words: the oracle's
    restatement of its splitter), and a start at every lead byte y of a three- or four-byte character behind a byte x that no
    merge joins it to (bit y - 0xE0 of seams[x] clear; k_tiles, "Seams")."""
    starts = set(split_words(doc))
    if doc:
        starts.add(0)
    if seams is not None:
        for i in range(1, len(doc)):
            y = doc[i]
            if y >= 0xE0 and not (seams[doc[i - 1]] >> (y & 31)) & 1:
                starts.add(i)
    s = sorted(starts) + [len(doc)]
    return [(a, b) for a, b in zip(s, s[1:]) if b > a]


def own_units(k, word):
    """Units of the word's own bytes: bytes (byte mode) or characters, an item of several units counted as those."""
    if k.is_byte:
        return sum(k.scale.get(b, 1) for b in word)
    return sum(k.scale.get(b, 1) for b in word if (b & 0xC0) != 0x80)


def gets_prefix(k, doc, start):
    """The document's first word gets the prefix units in front, unless the document begins with a space (then the prefix
    is a word of its own)."""
    return bool(k.prefix) and start == 0 and doc[:1] != b" "


def units(k, doc, start, end):
    return own_units(k, doc[start:end]) + (k.n_prefix if gets_prefix(k, doc, start) else 0)


def list_of(k, n):
    """exc_list_of: the list of a word of n = bytes + prefix units (the prefix counted whether or not the word gets it)."""
    quad_ok = (k.is_byte or not k.sym32) and k.rank_is_sym and not k.multi
    group_ok = (not k.sym32) and k.rank_is_sym and not k.multi
    if quad_ok and n <= 128:
        return 0
    if quad_ok and n <= 256:
        return 1
    if group_ok and n <= 512:
        return 2
    if group_ok and n <= 1024:
        return 3
    return 4


def word_list(k, doc, start, end):
    """-> the list (0..4) the word goes on, None when it goes on none, "?" where that depends on how its tile is filled.
    Beyond 63 bytes every word is an exception word and is listed by its bytes + prefix units.  Up to 63 bytes a word is an
    exception word when it has more than 32 units (or, with items of several units, holds such an item); d_exc_lane /
    d_exc_medium then encode it themselves unless the vocabulary has items of several units or prefix + bytes pass 64."""
    nb = end - start
    if nb > LANE_MAX_BYTES:
        return list_of(k, nb + k.n_prefix)
    kp = k.n_prefix if gets_prefix(k, doc, start) else 0
    if k.multi:  # (every exception word is d_exc's, which expands the items)
        has_item = any(b in k.scale for b in doc[start:end])
        if has_item or own_units(k, doc[start:end]) + kp > LANE_MAX_UNITS:
            return 4
        # (character mode: a document's first word is an exception word too when its tile's room for prefixes is used up)
        return "?" if k.prefix and start == 0 else None
    if kp + nb > MEDIUM_UNITS:
        return list_of(k, nb + k.n_prefix) if own_units(k, doc[start:end]) + kp > LANE_MAX_UNITS else "?"
    return None


ARENA_WORDS, RUN_EXTRA = 4, 64  # per tile: document-first words k_tiles gives prefix units in front, and its room for prefix units / ids


def is_exception_word(k, doc, start, end):
    """Does k_tiles hand the word over as an exception record whatever else its tile holds?  More than 63 bytes, more than
    32 units with the prefix, or an item of several units."""
    kp = k.n_prefix if gets_prefix(k, doc, start) else 0
    return (end - start > LANE_MAX_BYTES or own_units(k, doc[start:end]) + kp > LANE_MAX_UNITS
            or (k.multi and any(b in k.scale for b in doc[start:end])))


def list_counts(k, docs, seams, split_words):
    """-> ([words on list 0..4], words whose list the restatement cannot tell, [(doc, start, end, list)] of the listed)

    Character mode with items of several units: a document's first word of up to 63 bytes without an item asks its tile
    (the one its first byte is in) for one of ARENA_WORDS places before its units are counted; those that get none are
    exception words, and d_exc's as every exception word of such a vocabulary.  Which of a tile's candidates go without is
    not defined, but how many is: the candidates beyond four.  They add to the wave list unless they are on it anyway for
    their more than 32 units -- so the count is exact for a tile with at most four candidates, or with none of more than
    32 units; any other tile's candidates are "cannot tell".  (The room for prefix units, RUN_EXTRA, is never used up by
    four words and the documents that begin with a space: checked.)"""
    counts, unknown, listed = [0] * 5, 0, []
    tiles, base = {}, 0  # tile -> [candidates of at most 32 units, of more, documents that begin with a space]
    for d, doc in enumerate(docs):
        for a, b in gpu_words(doc, seams, split_words):
            li = word_list(k, doc, a, b)
            if k.multi and k.prefix and a == 0 and b - a <= LANE_MAX_BYTES and not any(c in k.scale for c in doc[a:b]):
                t = tiles.setdefault(base // TILE, [0, 0, 0])
                t[2 if doc[:1] == b" " else 1 if li == 4 else 0] += 1
                li = None if li == "?" else li
            if li == "?":
                unknown += 1
            elif li is not None:
                counts[li] += 1
                listed.append((d, a, b, li))
        base += len(doc)
    for few, many, spaced in tiles.values():
        over = few + many - ARENA_WORDS
        if spaced * k.n_prefix + ARENA_WORDS * k.n_prefix > RUN_EXTRA or (over > 0 and few and many):
            unknown += few + many + spaced
        elif over > 0 and few:
            counts[4] += over
    return counts, unknown, listed


def wave_lds_route(k, n_units, small):
    """Where d_exc merges a word of n_units: "lds" or "hbm".  k_exc_b<true> (16-bit symbols, rank == symbol order) calls
    d_exc<2048>: up to 2046 units in LDS; everything else, k_tail_small included, d_exc<1024>."""
    fast = (not k.sym32) and k.rank_is_sym
    return "lds" if n_units <= (2046 if fast and not small else 1024) else "hbm"


# ---- words ----------------------------------------------------------------------------------------------------

SINGLES = {"1": LETTERS_1[:6], "12": LETTERS_1[:6] + LETTERS_2, "3": LETTERS_3}


def _glue(k, rng, n_units, cls="1", piece_p=0.7):
    """A word of exactly n_units own units glued from the kind's keys of one class of letters (the last key cut to fit), no
    item of several units.  cls: "1" ASCII letters, "12" with two-byte letters (one word for the splitter, bytes != units),
    "3" three-byte characters only (a word of their own for the splitter).  The word stays ONE word for k_tiles: no key
    follows a byte that the seam map cuts its lead byte from, nor holds such a pair of bytes itself, and a word of
    class "12" begins and ends with an ASCII letter."""
    pieces, singles = k.pieces[cls], SINGLES[cls]
    parts, have, last, tries, stuck = [], 0, None, 0, 0
    while have < n_units:
        tries += 1
        stuck += 1
        assert tries < 400 * n_units + 4000, (k.tag, cls, n_units)
        if stuck > 200 and parts:  # (nothing may follow the last key: take it back)
            have -= len(parts.pop())
            last = parts[-1].encode("utf-8")[-1] if parts else None
            stuck = 0
        p = rng.choice(pieces) if pieces and rng.random() < piece_p else rng.choice(singles)
        p = p[: n_units - have]
        if cls == "12" and (last is None or have + len(p) == n_units):
            if last is None and ord(p[0]) >= 0x80:
                continue
            if have + len(p) == n_units and ord(p[-1]) >= 0x80:
                p = p[:-1] + rng.choice(SINGLES["1"])
        b = p.encode("utf-8")
        if k.seams is not None and any(y >= 0xE0 and not (k.seams[x] >> (y & 31)) & 1
                                       for x, y in (zip(b, b[1:]) if last is None else zip(bytes([last]) + b, b))):
            continue
        parts.append(p)
        have += len(p)
        last = b[-1]
        stuck = 0
    return "".join(parts).encode("utf-8")


def word(k, rng, n_units, items=0, at=None, cls="1", piece_p=0.7):
    """A word of n_units own units.  items: that many q's inside it (q -> "Alpha", five units: the bytes stay below the
    units), put in the place of one-byte letters; at: byte positions for them (words of ASCII letters)."""
    if k.is_byte:
        cls = "1"
    if not items:
        return _glue(k, rng, n_units, cls, piece_p)
    extra = k.scale[ord("q")] - 1
    base = bytearray(_glue(k, rng, n_units - extra * items, "1" if at is not None or cls == "3" else cls, piece_p))
    free = [i for i, b in enumerate(base) if b < 0x80]
    assert len(free) >= items
    spots = at if at is not None else rng.sample(free, items)
    for p in spots:
        base[p] = ord("q")
    return bytes(base)


def _long_units(k, doc):
    return [units(k, doc, x, y) for x, y in gpu_words(doc, k.seams, _split())]


def _split():
    from oracle import oracle as O
    return O.split_words


def limit_docs(k, seed=1):
    """-> [(document, form, limit, class)]: for every limit and every position form a document whose long word has exactly
    that many units (prefix included where the word gets one; a leading space is a unit of the word where the splitter
    gives it to the word).  Character kinds take the classes of letters in turn; kinds with q -> "Alpha" come with 0, 1,
    2 and 13 such items per word."""
    if ("limits", k.tag, seed) in _docs:
        return _docs[("limits", k.tag, seed)]
    rng = random.Random(seed * 1000 + sorted(KINDS).index(k.tag))
    out = []
    short = lambda: word(k, rng, rng.randint(2, 5))
    n_items = (0, 1, 2, 13) if k.multi else (0,)
    turn = ("12", "3", "1", "12", "3", "12", "1")
    for li, u in enumerate(LIMITS):
        for fi, form in enumerate(FORMS):
            for it in n_items:
                cls = "1" if k.is_byte else turn[(li + 2 * fi) % len(turn)]
                docfirst = form in ("alone", "short-behind", "long-behind")
                if it and (u - (k.n_prefix + 1) - 4 * it < it or form not in ("alone", "behind-short")):
                    continue
                base = u - (k.n_prefix if docfirst and k.prefix else 0)
                for own in (base - (0 if docfirst else 1), base) * 6:  # (the second: a seam leaves the space a word of its own)
                    w = word(k, rng, own, items=it, cls=cls)
                    if form == "alone":
                        doc = w
                    elif form == "space-first":
                        doc = b" " + w
                    elif form == "behind-short":
                        doc = short() + b" " + w
                    elif form == "short-behind":
                        doc = w + b" " + short()
                    else:
                        doc = w + b" " + word(k, rng, max(u - 1, 2), cls="1")
                    if u in _long_units(k, doc):
                        break
                else:
                    raise AssertionError((k.tag, form, u, cls, doc[:80]))
                out.append((doc, form, u, cls))
    _docs[("limits", k.tag, seed)] = out
    return out


def item_place_docs(k, rng):
    """Items of several units at bytes 0, 63, 64 and last of a 64-byte step of d_exc's expansion loop, and documents of
    nothing but such items (more ids than bytes per tile)."""
    docs = []
    if k.multi and ord("q") in k.scale:
        for n in (65, 128, 200, 1030):
            for at in ([0], [63], [64], [-1], [0, 63, 64, -1]):
                docs.append(word(k, rng, n + 4 * len(at), items=len(at), at=at))
        docs += [b"q" * 5000, b"aqb " * 2000, b"q" * 13 + b"e" * 47]
    if ord("\t") in k.scale:
        docs += [b"\t" * 5000, b"a\tb " * 2000, b"\n" * 300 + b"ab\t\tcd\n"]
    return docs


def tile_end_docs(k, rng):
    """helpers.later_tile_word_docs' forms on glued words: a word that starts `lead` bytes into its document and ends in the
    same tile or one to three tiles on, at the document's end, with a short or a long word behind."""
    docs = []
    for lead in (0, 1, 500, 897, 959, 961):
        for n in (65, 959 - lead % 960 if 959 - lead % 960 >= 64 else 100, 960, 1025, 1921, 2880):
            pre = (word(k, rng, lead - 1) + b" ") if lead > 1 else (b" " if lead else b"")
            w = word(k, rng, n)
            docs += [pre + w, pre + w + b" " + word(k, rng, 3), pre + w + b" " + word(k, rng, n)]
    return docs


def mixed_docs(k, rng):
    """Words for every list in ONE document each (a small batch then holds entries of all of the kind's lists at once)."""
    return [b" ".join(word(k, rng, n, cls=c) for n, c in zip(ns, ("1", "12", "3", "12", "1", "1")))
            for ns in ((100, 200, 400, 800, 1500, 40), (1100, 129, 65, 513, 257, 33))]


def _first_word_class(k, doc):
    """0 / 2: the document's first word asks its tile for a place for prefix units and has at most / more than 32 units
    (list_counts); 1: it does not ask."""
    a, b = gpu_words(doc, k.seams, _split())[0]
    if b - a > LANE_MAX_BYTES or doc[:1] == b" " or any(c in k.scale for c in doc[a:b]):
        return 1
    return 2 if own_units(k, doc[a:b]) + k.n_prefix > LANE_MAX_UNITS else 0


def full_docs(k):
    """Every document of the kind, the batch of the full tail (well past 32 tiles); the last one is a long word.
    Character mode with items of several units: the documents whose first word asks for prefix room come first where it has
    at most 32 units and last where it has more, with the others (hundreds of tiles) between them, so that no tile holds
    both and list_counts can tell every word's list."""
    if k.tag not in _docs:
        rng = random.Random(7000 + sorted(KINDS).index(k.tag))
        docs = [d for d, _f, _u, _c in limit_docs(k)] + item_place_docs(k, rng) + tile_end_docs(k, rng) + mixed_docs(k, rng)
        if k.multi and k.prefix:
            docs.sort(key=lambda d: _first_word_class(k, d))
        docs.append(word(k, rng, 70))
        _docs[k.tag] = docs
    return _docs[k.tag]


def giant_docs(k):
    """Two documents with a word of GIANT[0] and of GIANT[1] units: one key in seven pieces, the rest single letters (about
    a tenth of the units merge away: the reference's merge loop is quadratic in them)."""
    rng = random.Random(8000 + sorted(KINDS).index(k.tag))
    it = 3 if k.multi else 0
    return [word(k, rng, GIANT[0] - (k.n_prefix if k.prefix else 0), items=it, cls="12", piece_p=0.15),
            b"x " + word(k, rng, GIANT[1] - 1, items=it, cls="12", piece_p=0.15)]


def tiles_of(docs):
    return (sum(len(d) for d in docs) + TILE - 1) // TILE


def small_batches(docs):
    """The documents cut into consecutive batches of 5..32 tiles and at most 4096 documents (k_tail_small's), in order;
    a document that cannot share a batch within those limits -- it is longer than 32 tiles, or what is left is too short
    -- is left out (returned second)."""
    out, left_out, cur, size = [], [], [], 0
    lo, hi = 5 * TILE - TILE + 1, SMALL_TILES * TILE
    target = 12 * TILE
    for d in docs:
        if len(d) > hi:
            left_out.append(d)
            continue
        if cur and (size + len(d) > hi or len(cur) == SMALL_DOCS):
            out.append(cur)
            cur, size = [], 0
        cur.append(d)
        size += len(d)
        if size >= target:
            out.append(cur)
            cur, size = [], 0
    if cur:
        if size >= lo:
            out.append(cur)
        elif out and tiles_of(out[-1] + cur) <= SMALL_TILES and len(out[-1]) + len(cur) <= SMALL_DOCS:
            out[-1] = out[-1] + cur
        else:
            left_out += cur
    return out, left_out


def one_launch_batches(k):
    """Each limit word of up to ONE_LAUNCH_MAX bytes alone, and with one short neighbour, in a batch of at most four tiles."""
    out = []
    for doc, form, _u, _c in limit_docs(k):
        if form in ("alone", "behind-short", "space-first") and len(doc) <= ONE_LAUNCH_MAX:
            out.append([doc])
            if form == "alone":
                out.append([b"ab", doc])
    return out
