"""Tables of the GPU WordPiece encoder (csrc/hutk_wordpiece.hip, csrc/hutk_wordpiece.h), built from this interpreter's
`unicodedata`: the character classes of BERT's normaliser and word split, and the lower-case mapping of every code
point.  Nothing here tokenises text.

The blob (little-endian 32-bit words; every offset is in bytes from the blob's start and a multiple of 4; the same
layout is documented in include/hutoken_amd.h):

  header, 32 words
    0 magic "HWPC" (0x43505748)   1 format version (1)      2 unidata_version as major << 16 | minor << 8 | patch
    3 size of the blob in bytes
    4, 5   stage one: offset, entries       uint16[0x110000 >> 7]: the block of code point c is stage1[c >> 7]
    6, 7   class blocks: offset, blocks     one word per code point, 128 code points per block:
             bits 0..2   class under clean_text: 0 word, 1 space, 2 punctuation, 3 CJK, 4 dropped, 5 nonspacing mark
             bits 3..23  the lower-case mapping's first character less the code point, modulo 2^21 (0: no mapping)
             bits 24..26 class without clean_text (what clean_text drops is then a word character or a space)
             bits 27..31 index of the mapping's second character in the table below, 0: the mapping is one character
    8, 9   second characters: offset, entries   uint32, entry 0 unused
    10     the block shift (7)
    16..19 largest (characters out) / (bytes in) of one code point through the fold, rounded up, for the settings
           lowercase | strip_accents << 1: what hutk_wordpiece_ids_capacity multiplies n_bytes by
    20..23 largest (bytes out) / (bytes in) of one code point through the fold, times 16, rounded up, same settings:
           what the folded text's workspace is sized by

`python -m hutoken_amd.wordpiece --write FILE` writes the blob for C integrators (hutk_wordpiece_create).
"""
import struct
import sys
import unicodedata

MAGIC, VERSION = 0x43505748, 1
BLOCK_SHIFT = 7
HEADER_WORDS = 32
WORD, SPACE, PUNCT, CJK, DROPPED, MARK = range(6)
CLEAN_TEXT, CJK_CHARS, STRIP_ACCENTS, LOWERCASE = 1, 2, 4, 8  # HUTK_WP_*
WHITE_SPACE = frozenset([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]
                        + list(range(0x2000, 0x200B)))
# (the sixth range starts at U+2B920 as in the `tokenizers` package, not at U+2B820 as in Google's BERT)
CJK_RANGES = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F),
              (0x2B920, 0x2CEAF), (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))

_blob = None
_facts = None


def flags_of(lowercase=True, strip_accents=None, clean_text=True, handle_chinese_chars=True):
    """The four options of BertNormalizer -> the HUTK_WP_* flag word; strip_accents=None: as lowercase."""
    for name, v in (("lowercase", lowercase), ("clean_text", clean_text), ("handle_chinese_chars", handle_chinese_chars)):
        if not isinstance(v, bool):
            raise TypeError("%s must be a bool, not %s" % (name, type(v).__name__))
    if strip_accents is not None and not isinstance(strip_accents, bool):
        raise TypeError("strip_accents must be a bool or None, not %s" % type(strip_accents).__name__)
    if strip_accents is None:
        strip_accents = lowercase
    return (CLEAN_TEXT if clean_text else 0) | (CJK_CHARS if handle_chinese_chars else 0) | \
        (STRIP_ACCENTS if strip_accents else 0) | (LOWERCASE if lowercase else 0)


def _build():
    import numpy as np
    n_cp = 0x110000
    cat = unicodedata.category
    clean = np.zeros(n_cp, dtype=np.uint32)
    plain = np.zeros(n_cp, dtype=np.uint32)
    lower = np.zeros(n_cp, dtype=np.uint32)
    second = np.zeros(n_cp, dtype=np.uint32)
    seconds = [0]
    for c in range(n_cp):
        if 0xD800 <= c < 0xE000:  # strict UTF-8 rejects an encoded surrogate: none is ever looked up
            continue
        ch = chr(c)
        k = cat(ch)
        if c in WHITE_SPACE:
            a = b = SPACE
        elif k[0] == "P" or 33 <= c <= 47 or 58 <= c <= 64 or 91 <= c <= 96 or 123 <= c <= 126:
            a = b = PUNCT
        elif k == "Mn":
            a = b = MARK
        elif any(lo <= c <= hi for lo, hi in CJK_RANGES):
            a = b = CJK
        else:
            a = b = WORD
        if c in (0x09, 0x0A, 0x0D):
            pass
        elif c == 0 or c == 0xFFFD or k in ("Cc", "Cf", "Co"):
            a = DROPPED
        clean[c], plain[c] = a, b
        low = ch.lower()
        if low != ch:
            assert 1 <= len(low) <= 2, "a lower-case mapping of %d characters" % len(low)
            lower[c] = (ord(low[0]) - c) & 0x1FFFFF
            if len(low) == 2:
                o = ord(low[1])
                if o not in seconds:
                    seconds.append(o)
                second[c] = seconds.index(o)
    assert len(seconds) < 32, "second characters are indexed by 5 bits"
    words = clean | (lower << 3) | (plain << 24) | (second << 27)

    def fold(c, low, strip):
        out = unicodedata.normalize("NFD", chr(c)) if strip else chr(c)
        if strip:
            out = "".join(x for x in out if cat(x) != "Mn")
        if low:
            out = "".join(x.lower() for x in out)
        return out

    char_ratio, byte_ratio16 = [1] * 4, [16] * 4
    special = [c for c in range(n_cp) if not 0xD800 <= c < 0xE000 and
               (chr(c).lower() != chr(c) or unicodedata.decomposition(chr(c)) or 0xAC00 <= c < 0xAC00 + 11172)]
    for c in special:
        src = len(chr(c).encode("utf-8"))
        for s in range(4):
            out = fold(c, bool(s & 1), bool(s & 2))
            char_ratio[s] = max(char_ratio[s], -(-len(out) // src))
            byte_ratio16[s] = max(byte_ratio16[s], -(-16 * len(out.encode("utf-8")) // src))

    bs = 1 << BLOCK_SHIFT
    rows = words.reshape(n_cp >> BLOCK_SHIFT, bs)
    blocks, stage1, kept = {}, [], []
    for b in range(n_cp >> BLOCK_SHIFT):
        key = rows[b].astype("<u4").tobytes()
        at = blocks.get(key)
        if at is None:
            at = blocks[key] = len(blocks)
            kept.append(key)
        stage1.append(at)
    assert len(blocks) < 65536
    uv = [int(x) for x in unicodedata.unidata_version.split(".")] + [0, 0]
    head = [0] * HEADER_WORDS
    off = 4 * HEADER_WORDS
    s1 = struct.pack("<%dH" % len(stage1), *stage1)
    s1 += b"\0" * (-len(s1) % 4)
    cl = b"".join(kept)
    sc = struct.pack("<%dI" % len(seconds), *seconds)
    head[4], head[5] = off, len(stage1)
    off += len(s1)
    head[6], head[7] = off, len(blocks)
    off += len(cl)
    head[8], head[9] = off, len(seconds)
    off += len(sc)
    head[0], head[1], head[2], head[3] = MAGIC, VERSION, uv[0] << 16 | uv[1] << 8 | uv[2], off
    head[10] = BLOCK_SHIFT
    head[16:20] = char_ratio
    head[20:24] = byte_ratio16
    blob = struct.pack("<%dI" % HEADER_WORDS, *head) + s1 + cl + sc
    assert len(blob) == off
    facts = {"unidata_version": unicodedata.unidata_version, "char_ratio": char_ratio, "byte_ratio16": byte_ratio16,
             "seconds": seconds, "blocks": len(blocks), "bytes": len(blob)}
    return blob, facts


def table_blob():
    """The blob (bytes), built at the first call of the process."""
    global _blob, _facts
    if _blob is None:
        _blob, _facts = _build()
    return _blob


def table_facts():
    """What the builder found on the way (tests assert it against unicodedata)."""
    table_blob()
    return _facts


def entry(blob, c):
    """The class word of code point c, read the way the kernels read it."""
    head = struct.unpack_from("<%dI" % HEADER_WORDS, blob, 0)
    b = struct.unpack_from("<H", blob, head[4] + 2 * (c >> BLOCK_SHIFT))[0]
    return struct.unpack_from("<I", blob, head[6] + 4 * ((b << BLOCK_SHIFT) | (c & ((1 << BLOCK_SHIFT) - 1))))[0]


def lower_of(blob, c):
    """The lower-case mapping of code point c as the kernels read it: a str of one or two characters."""
    e = entry(blob, c)
    head = struct.unpack_from("<%dI" % HEADER_WORDS, blob, 0)
    out = chr((c + ((e >> 3) & 0x1FFFFF)) & 0x1FFFFF)
    if e >> 27:
        out += chr(struct.unpack_from("<I", blob, head[8] + 4 * (e >> 27))[0])
    return out


def validate_blob(blob):
    """What hutk_wordpiece_create checks before anything reads through the blob, restated; -> None or the reason."""
    if len(blob) < 4 * HEADER_WORDS or len(blob) % 4:
        return "the blob is shorter than its header or no multiple of 4 bytes"
    h = struct.unpack_from("<%dI" % HEADER_WORDS, blob, 0)
    if h[0] != MAGIC or h[1] != VERSION:
        return "wrong magic or version"
    if h[3] != len(blob) or h[10] != BLOCK_SHIFT:
        return "wrong size or block shift"
    if h[5] != 0x110000 >> BLOCK_SHIFT or h[7] < 1 or h[7] > 65535 or h[9] < 1 or h[9] > 32:
        return "wrong section sizes"
    for off, n in ((h[4], 2 * h[5]), (h[6], 4 * h[7] << BLOCK_SHIFT), (h[8], 4 * h[9])):
        if off % 4 or off < 4 * HEADER_WORDS or off + n > len(blob):
            return "a section lies outside the blob"
    if any(b >= h[7] for b in struct.unpack_from("<%dH" % h[5], blob, h[4])):
        return "a stage-one entry names a block the blob does not hold"
    import numpy as np
    stage1 = np.frombuffer(blob, dtype="<u2", count=h[5], offset=h[4]).astype(np.int64)
    words = np.frombuffer(blob, dtype="<u4", count=h[7] << BLOCK_SHIFT, offset=h[6]).reshape(h[7], 1 << BLOCK_SHIFT)
    w = words[stage1].reshape(-1).astype(np.int64)  # the word of every code point
    low = (np.arange(0x110000, dtype=np.int64) + ((w >> 3) & 0x1FFFFF)) & 0x1FFFFF
    if ((w & 7) > MARK).any() or (((w >> 24) & 7) > MARK).any() or (low >= 0x110000).any() or ((w >> 27) >= h[9]).any():
        return "a class word holds a class, a code point or an index out of range"
    if any(s >= 0x110000 for s in struct.unpack_from("<%dI" % h[9], blob, h[8])):
        return "a second character is no code point"
    if any(not 1 <= r <= 4 for r in h[16:20]) or any(not 16 <= r <= 64 for r in h[20:24]):
        return "a ratio out of range"
    return None


def _main(argv):
    if len(argv) == 2 and argv[0] == "--write":
        blob = table_blob()
        with open(argv[1], "wb") as f:
            f.write(blob)
        print("%s: %d bytes, Unicode %s" % (argv[1], len(blob), unicodedata.unidata_version))
        return 0
    print("usage: python -m hutoken_amd.wordpiece --write FILE", file=sys.stderr)
    return 2


if __name__ == "__main__":
    sys.exit(_main(sys.argv[1:]))
