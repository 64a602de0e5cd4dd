"""Tables of the GPU normaliser (csrc/hutk_normalize.hip, csrc/hutk_norm.h), built from this interpreter's
`unicodedata`: one blob for the four forms NFC, NFD, NFKC, NFKD.  Nothing here normalises text.

The blob (little-endian 32-bit words; every offset is in bytes from the blob's start and a multiple of 4; the same
layout is documented in include/hutoken_amd.h):

  header, 32 words
    0 magic "HNRM" (0x4D524E48)   1 format version (1)      2 unidata_version as major << 16 | minor << 8 | patch
    3 size of the blob in bytes
    4, 5   stage one: offset, entries      uint16[0x110000 >> 7]: the block of code point c is stage1[c >> 7]
    6, 7   property blocks: offset, blocks  two words per code point, 128 code points per block:
             word 0: bits 0..7 ccc | bit 8 + f: quick check "Yes" under form f | bit 12: can be the second of a
                     composite pair | bits 16..23 (24..31): ccc of the first character of the full canonical
                     (compatibility) decomposition
             word 1: bits 0..15 (16..31): word index of the canonical (compatibility) decomposition, 0: none
    8, 9   decompositions: offset, words    word 0 unused; an entry is its length n (1..18), then n words
                                            code point | second-of-a-pair << 21 | ccc << 24, fully expanded
    10, 11 composite pairs: offset, slots   open addressing, a power of two of slots of four words {a, b, composite, 0},
                                            a == 0xFFFFFFFF: empty; slot = pair_hash(a, b) & (slots - 1), linear probing
    12 pairs in the table                   13 the block shift (7)
    16..19 first lead byte that can start an unstable character, per form (NFC, NFD, NFKC, NFKD)
    20..23 largest output / input byte ratio of one character, per form, rounded up
    24..27 first unstable code point, per form
  Hangul syllables and jamo are composed and decomposed arithmetically: they have no decomposition entries.

`python -m hutoken_amd.normalize --write FILE` writes the blob for C integrators (hutk_normalizer_create).
"""
import struct
import sys
import unicodedata

FORMS = ("NFC", "NFD", "NFKC", "NFKD")
MAGIC, VERSION = 0x4D524E48, 1
BLOCK_SHIFT = 7
HEADER_WORDS = 32
EMPTY = 0xFFFFFFFF
S_BASE, S_COUNT, L_BASE, V_BASE, T_BASE = 0xAC00, 11172, 0x1100, 0x1161, 0x11A7

_blob = None
_facts = None


def form_index(form):
    """"NFC" .. "NFKD" -> 0 .. 3 (the C ABI's HUTK_NFC ..); anything else raises."""
    if not isinstance(form, str):
        raise TypeError("form must be one of %s, not %s" % (", ".join(FORMS), type(form).__name__))
    if form not in FORMS:
        raise ValueError("form must be one of %s, not %r" % (", ".join(FORMS), form))
    return FORMS.index(form)


def pair_hash(a, b):
    return (((a * 31 + b) & 0xFFFFFFFF) * 0x9E3779B1 & 0xFFFFFFFF) >> 12


def _scalars():
    for c in range(0x110000):
        if not 0xD800 <= c < 0xE000:
            yield c


def _build():
    import numpy as np
    norm = unicodedata.normalize
    n_cp = 0x110000
    cps = [c for c in range(n_cp) if not 0xD800 <= c < 0xE000]
    chars = list(map(chr, cps))
    ccc = np.zeros(n_cp, dtype=np.uint8)
    ccc[cps] = np.fromiter(map(unicodedata.combining, chars), dtype=np.uint8, count=len(chars))
    # a form changes a character only when it has a decomposition mapping or is a Hangul syllable
    raws = list(map(unicodedata.decomposition, chars))
    cand = [cps[i] for i in np.flatnonzero(np.array(raws, dtype=bool))] + list(range(S_BASE, S_BASE + S_COUNT))
    changed = [{c: out for c in cand if (out := norm(name, chr(c))) != chr(c)} for name in FORMS]
    full = [{}, {}]  # canonical, compatibility: code point -> tuple of code points (only where it differs)
    pairs = {}
    for which, f in ((0, 1), (1, 3)):
        for c, out in changed[f].items():
            if not S_BASE <= c < S_BASE + S_COUNT:
                full[which][c] = tuple(map(ord, out))
    for c in full[0]:
        raw = unicodedata.decomposition(chr(c))
        parts = [int(x, 16) for x in raw.split()]
        # unicodedata does not expose the composition exclusions: a primary composite is a two-character canonical
        # decomposition that NFC puts together again
        if len(parts) == 2 and norm("NFC", changed[1][c]) == chr(c):
            pairs[(parts[0], parts[1])] = c
    second = set(b for _a, b in pairs)
    second.update(range(V_BASE, V_BASE + 21))
    second.update(range(T_BASE + 1, T_BASE + 28))

    def entry(c):
        return c | ((1 << 21) if c in second else 0) | (int(ccc[c]) << 24)

    pool = [0]
    index = [{}, {}]
    seen = {}
    for which in (0, 1):
        for c, seq in full[which].items():
            if which == 1 and full[0].get(c) == seq:
                index[1][c] = index[0][c]
                continue
            at = seen.get(seq)
            if at is None:
                at = seen[seq] = len(pool)
                pool.append(len(seq))
                pool.extend(entry(x) for x in seq)
            index[which][c] = at
    assert len(pool) < 65536, "decomposition indices are 16 bits"

    # the property words: a stable starter by default, the rest one by one
    w0s = ccc.astype(np.uint32) | np.uint32(0xF << 8)
    w1s = np.zeros(n_cp, dtype=np.uint32)
    special = set(np.flatnonzero(ccc).tolist()) | second
    for ch in changed:
        special.update(ch)
    first = [n_cp] * 4
    ratio = [1] * 4
    for c in special:
        hangul = S_BASE <= c < S_BASE + S_COUNT
        can = (L_BASE + (c - S_BASE) // 588,) if hangul else full[0].get(c, (c,))
        com = can if hangul else full[1].get(c, (c,))
        qc = 0
        src = len(chr(c).encode("utf-8"))
        for f in range(4):
            out = changed[f].get(c)
            yes = out is None and not ((f & 1) == 0 and c in second)
            qc |= yes << f
            if out is not None:
                ratio[f] = max(ratio[f], -(-len(out.encode("utf-8")) // src))
            lead = ccc[(com if f & 2 else can)[0]]
            if c < first[f] and not (yes and ccc[c] == 0 and lead == 0):
                first[f] = c
        w0s[c] = int(ccc[c]) | (qc << 8) | ((c in second) << 12) | (int(ccc[can[0]]) << 16) | (int(ccc[com[0]]) << 24)
        w1s[c] = index[0].get(c, 0) | (index[1].get(c, index[0].get(c, 0)) << 16)
    # (U+D800..U+DFFF keep the default: strict UTF-8 rejects an encoded surrogate, so none is ever looked up)

    bs = 1 << BLOCK_SHIFT
    both = np.stack([w0s, w1s], axis=1).reshape(n_cp >> BLOCK_SHIFT, 2 * bs)
    blocks, stage1, kept = {}, [], []
    for b in range(n_cp >> BLOCK_SHIFT):
        key = both[b].tobytes()
        at = blocks.get(key)
        if at is None:
            at = blocks[key] = len(blocks)
            kept.append(key)
        stage1.append(at)
    assert len(blocks) < 65536

    slots = 1
    while slots < 2 * len(pairs) + 2:
        slots *= 2
    table = [EMPTY, EMPTY, EMPTY, 0] * slots
    for (a, b), c in sorted(pairs.items()):
        s = pair_hash(a, b) & (slots - 1)
        while table[4 * s] != EMPTY:
            s = (s + 1) & (slots - 1)
        table[4 * s:4 * s + 4] = [a, b, c, 0]

    uv = [int(x) for x in unicodedata.unidata_version.split(".")] + [0, 0]
    head = [0] * HEADER_WORDS
    off = 4 * HEADER_WORDS
    s1 = struct.pack("<%dH" % len(stage1), *stage1)
    s1 += b"\0" * (-len(s1) % 4)
    pr = b"".join(kept)
    dc = struct.pack("<%dI" % len(pool), *pool)
    cm = struct.pack("<%dI" % len(table), *table)
    head[4], head[5] = off, len(stage1)
    off += len(s1)
    head[6], head[7] = off, len(blocks)
    off += len(pr)
    head[8], head[9] = off, len(pool)
    off += len(dc)
    head[10], head[11] = off, slots
    off += len(cm)
    head[0], head[1], head[2], head[3] = MAGIC, VERSION, uv[0] << 16 | uv[1] << 8 | uv[2], off
    head[12], head[13] = len(pairs), BLOCK_SHIFT
    for f in range(4):
        head[16 + f] = chr(first[f]).encode("utf-8")[0]
        head[20 + f] = ratio[f]
        head[24 + f] = first[f]
    blob = struct.pack("<%dI" % HEADER_WORDS, *head) + s1 + pr + dc + cm
    assert len(blob) == off
    facts = {"unidata_version": unicodedata.unidata_version, "first_unstable": first,
             "first_lead": head[16:20], "max_expansion": ratio, "pairs": pairs, "ccc": ccc.tobytes(),
             "decomposition_words": len(pool), "blocks": len(blocks), "bytes": len(blob)}
    return blob, facts


def table_blob():
    """The blob (bytes), built at the first call of the process."""
    global _blob, _facts
    if _blob is None:
        _blob, _facts = _build()
    return _blob


def table_facts():
    """What the builder found on the way (tests assert it against unicodedata): first unstable code points and lead
    bytes and the largest expansions per form, the composite pairs, the ccc of every code point."""
    table_blob()
    return _facts


def _main(argv):
    if len(argv) == 2 and argv[0] == "--write":
        blob = table_blob()
        with open(argv[1], "wb") as f:
            f.write(blob)
        print("%s: %d bytes, Unicode %s" % (argv[1], len(blob), unicodedata.unidata_version))
        return 0
    print("usage: python -m hutoken_amd.normalize --write FILE", file=sys.stderr)
    return 2


if __name__ == "__main__":
    sys.exit(_main(sys.argv[1:]))
