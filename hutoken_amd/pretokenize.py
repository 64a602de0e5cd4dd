"""Tables of the GPU pre-tokeniser (csrc/hutk_presplit.hip, csrc/hutk_presplit.h), built from this interpreter's
`unicodedata`: the class of every code point -- letter (general category L*), number (N*), whitespace (the 25
White_Space code points) or other -- for the split presets gpt2, cl100k (alias llama3) and qwen2.  Nothing here splits
text.

The classes are those of the interpreter's Unicode version (`unicodedata.unidata_version`); a tokenizer library built on
a newer database counts the letters and numbers assigned since then as such, this table counts them as "other".

The blob (little-endian 32-bit words; every offset is in bytes from the blob's start and a multiple of 4; the same
layout is documented in include/hutoken_amd.h):

  header, 16 words
    0 magic "HPTK" (0x4B545048)   1 format version (1)      2 unidata_version as major << 16 | minor << 8 | patch
    3 size of the blob in bytes
    4, 5   stage one: offset, entries     uint16[0x110000 >> 7]: the block of code point c is stage1[c >> 7]
    6, 7   class blocks: offset, blocks   8 words a block, 128 code points of two bits: code point c is bits
                                          2 * (c & 15) .. of word (c & 127) >> 4; 0 other, 1 letter, 2 number, 3 whitespace
    8 the block shift (7)

`python -m hutoken_amd.pretokenize --write FILE` writes the blob for C integrators (hutk_pretokenizer_create).
"""
import struct
import sys
import unicodedata

PRESETS = ("gpt2", "cl100k", "qwen2")  # the C ABI's HUTK_PRESPLIT_GPT2 .. in this order
ALIASES = {"llama3": "cl100k"}
PATTERNS = {
    "gpt2": r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+",
    "cl100k": r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+",
    "qwen2": r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+",
}
WHITE_SPACE = frozenset([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]
                        + list(range(0x2000, 0x200B)))
MAGIC, VERSION = 0x4B545048, 1
BLOCK_SHIFT = 7
HEADER_WORDS = 16
OTHER, LETTER, NUMBER, SPACE = 0, 1, 2, 3

_blob = None


def preset_index(preset):
    """"gpt2", "cl100k" (or "llama3"), "qwen2" -> 0 .. 2; anything else raises."""
    if not isinstance(preset, str):
        raise TypeError("preset must be one of %s, not %s" % (", ".join(PRESETS), type(preset).__name__))
    preset = ALIASES.get(preset, preset)
    if preset not in PRESETS:
        raise ValueError("preset must be one of %s (or llama3), not %r" % (", ".join(PRESETS), preset))
    return PRESETS.index(preset)


def _build():
    import numpy as np
    n_cp = 0x110000
    cat = unicodedata.category
    cls = np.fromiter(({"L": LETTER, "N": NUMBER}.get(cat(chr(c))[0], OTHER) for c in range(n_cp)), dtype=np.uint8, count=n_cp)
    cls[sorted(WHITE_SPACE)] = SPACE
    bs = 1 << BLOCK_SHIFT
    shifts = (2 * np.arange(16, dtype=np.uint32))[None, :]
    words = (cls.reshape(-1, 16).astype(np.uint32) << shifts).sum(axis=1, dtype=np.uint32).reshape(n_cp >> BLOCK_SHIFT, bs // 16)
    blocks, stage1, kept = {}, [], []
    for b in range(n_cp >> BLOCK_SHIFT):
        key = words[b].astype("<u4").tobytes()
        at = blocks.get(key)
        if at is None:
            at = blocks[key] = len(blocks)
            kept.append(key)
        stage1.append(at)
    assert len(blocks) < 65536
    uv = [int(x) for x in unicodedata.unidata_version.split(".")] + [0, 0]
    s1 = struct.pack("<%dH" % len(stage1), *stage1)
    s1 += b"\0" * (-len(s1) % 4)
    bl = b"".join(kept)
    head = [0] * HEADER_WORDS
    off = 4 * HEADER_WORDS
    head[4], head[5] = off, len(stage1)
    off += len(s1)
    head[6], head[7] = off, len(blocks)
    off += len(bl)
    head[0], head[1], head[2], head[3], head[8] = MAGIC, VERSION, uv[0] << 16 | uv[1] << 8 | uv[2], off, BLOCK_SHIFT
    blob = struct.pack("<%dI" % HEADER_WORDS, *head) + s1 + bl
    assert len(blob) == off
    return blob


def table_blob():
    """The blob (bytes), built at the first call of the process."""
    global _blob
    if _blob is None:
        _blob = _build()
    return _blob


def _main(argv):
    if len(argv) == 2 and argv[0] == "--write":
        blob = table_blob()
        with open(argv[1], "wb") as f:
            f.write(blob)
        print("%s: %d bytes, Unicode %s" % (argv[1], len(blob), unicodedata.unidata_version))
        return 0
    print("usage: python -m hutoken_amd.pretokenize --write FILE", file=sys.stderr)
    return 2


if __name__ == "__main__":
    sys.exit(_main(sys.argv[1:]))
