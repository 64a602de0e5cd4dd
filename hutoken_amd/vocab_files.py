"""Writers for huToken's two text file formats and the GPT-2 byte alphabet.

Formats (reference README.md:269-319; writers hutoken.py:64-73, 88-97 and
scripts/convert.py:9-15):

  vocab file      one token per line:  0xHH0xHH... == <int id>\\n
                  (every line, the last one too, must end in '\\n':
                  lib.c:264-289 drops an unterminated final line)
  special file    one byte per line:   <decimal 0..255> == <utf-8 string>\\n
                  lines are read in 31-character chunks (lib.c:483)
"""

# bytes the GPT-2 byte encoder remaps (reference hutoken.py:15-20)
SPECIAL_BYTES = list(range(0, 33)) + list(range(127, 161)) + [173]


def bytes_to_unicode():
    """GPT-2's byte -> visible character table: printable Latin-1 bytes map to
    themselves, the other 68 bytes to U+0100.. in ascending byte order."""
    keep = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
    table = {b: chr(b) for b in keep}
    n = 0
    for b in range(256):
        if b not in table:
            table[b] = chr(256 + n)
            n += 1
    return table


def byte_token_order():
    """Byte values in GPT-2 id order (ids 0..255 of a GPT-2-shaped vocab)."""
    keep = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
    return keep + [b for b in range(256) if b not in set(keep)]


def encode_visible(raw: bytes, table=None) -> bytes:
    """Raw bytes -> UTF-8 of their GPT-2 visible characters (what a vocab key
    for those bytes looks like in a byte-encoder vocabulary)."""
    table = table or bytes_to_unicode()
    return "".join(table[b] for b in raw).encode("utf-8")


def hex_line(token: bytes, idx: int) -> str:
    return "".join("0x%02X" % b for b in token) + " == %d\n" % idx


def write_vocab_file(path, entries, encoding="ascii"):
    """entries: iterable of (token bytes, id)."""
    with open(path, "w", encoding=encoding) as f:
        for tok, idx in entries:
            f.write(hex_line(tok, idx))


def write_special_file(path, mapping):
    """mapping: {byte value: replacement str}."""
    with open(path, "w", encoding="utf-8") as f:
        for b in sorted(mapping):
            f.write("%d == %s\n" % (b, mapping[b]))


def gpt2_special_mapping():
    t = bytes_to_unicode()
    return {b: t[b] for b in SPECIAL_BYTES}


def llama_special_mapping():
    """SentencePiece/Llama-shaped special file: space -> U+2581, control bytes
    and DEL -> byte-fallback literals (what hutoken.py:88-97 writes for such a
    tokenizer)."""
    m = {32: "▁"}
    for b in list(range(0, 32)) + [127]:
        m[b] = "<0x%02X>" % b
    return m


def merge_tokens(pairs):
    """Byte strings of the symbols 256.. that merges (a, b) create: token(256 + k) = token(a) + token(b)."""
    toks = [bytes([b]) for b in range(256)]
    for a, b in pairs:
        toks.append(toks[int(a)] + toks[int(b)])
    return toks[256:]


def gpt2_vocab_text(pairs, end_of_text="<|endoftext|>"):
    """A GPT-2-shaped vocab file (tools/make_vocab.py): the 256 byte tokens in byte_token_order(), the merges in
    order, visible-encoded, then the end token (if any).  ids = line order."""
    t = bytes_to_unicode()
    lines = [hex_line(encode_visible(bytes([b]), t), i) for i, b in enumerate(byte_token_order())]
    for tok in merge_tokens(pairs):
        lines.append(hex_line(encode_visible(tok, t), len(lines)))
    if end_of_text:
        lines.append(hex_line(end_of_text.encode("utf-8"), len(lines)))
    return "".join(lines)


def gpt2_merges_text(pairs):
    """merges.txt: "#version: 0.2", then one visible-encoded "left right" line per merge."""
    t = bytes_to_unicode()
    toks = [bytes([b]) for b in range(256)] + merge_tokens(pairs)
    out = ["#version: 0.2\n"]
    for a, b in pairs:
        out.append(encode_visible(toks[int(a)], t).decode("utf-8") + " " +
                   encode_visible(toks[int(b)], t).decode("utf-8") + "\n")
    return "".join(out)


def gpt2_special_text():
    return "".join("%d == %s\n" % (b, s) for b, s in sorted(gpt2_special_mapping().items()))


def write_gpt2_files(out_dir, name, pairs, end_of_text="<|endoftext|>"):
    """<name>_vocab.txt, <name>_special.txt, <name>_merges.txt under out_dir -> dict of the three paths."""
    import os
    paths = {"vocab_file": os.path.join(out_dir, name + "_vocab.txt"),
             "special_file": os.path.join(out_dir, name + "_special.txt"),
             "merges_file": os.path.join(out_dir, name + "_merges.txt")}
    for key, text in (("vocab_file", gpt2_vocab_text(pairs, end_of_text)), ("special_file", gpt2_special_text()),
                      ("merges_file", gpt2_merges_text(pairs))):
        with open(paths[key], "w", encoding="utf-8", newline="") as f:
            f.write(text)
    return paths


def raw_vocab_text(pairs, vocab_size):
    """The vocabulary bpe_train / bbpe_train write: raw bytes, bytes 0x01..0xFF as ids 0..254, merge k as 255 + k;
    vocab_size lines at most (no 0x00 line: a document cannot hold one and the loader rejects it)."""
    toks = [bytes([b]) for b in range(1, 256)] + merge_tokens(pairs)
    return "".join(hex_line(tk, i) for i, tk in enumerate(toks[:vocab_size]))


# ---- SentencePiece/Llama shape (VL, tools/make_vocab.py; the trainer's "chars" mode) ----------------------------
LLAMA_FIXED_TOKENS = 259  # <unk>, <s>, </s> and the 256 byte-fallback tokens <0x00>..<0xFF>


def char_merge_tokens(alphabet, pairs):
    """Byte strings of the symbols A.. that merges (a, b) create over an alphabet of A characters."""
    toks = list(alphabet)
    for a, b in pairs:
        toks.append(toks[int(a)] + toks[int(b)])
    return toks[len(alphabet):]


def llama_vocab_text(alphabet, pairs):
    """A Llama-shaped vocab file (tools/make_vocab.py, VL): <unk>, <s>, </s>, <0x00>..<0xFF>, the alphabet, then the
    merge tokens in order.  ids = line order."""
    toks = [b"<unk>", b"<s>", b"</s>"] + [b"<0x%02X>" % b for b in range(256)]
    toks += list(alphabet) + char_merge_tokens(alphabet, pairs)
    return "".join(hex_line(tk, i) for i, tk in enumerate(toks))


def llama_special_text():
    return "".join("%d == %s\n" % (b, s) for b, s in sorted(llama_special_mapping().items()))


def llama_merges_bytes(alphabet, pairs):
    """merges.txt of a chars-mode run: "#version: 0.2", then one raw "left right" line per merge (no token holds a
    space or a newline: spaces became U+2581 and words with control bytes were dropped)."""
    toks = list(alphabet) + char_merge_tokens(alphabet, pairs)
    return b"#version: 0.2\n" + b"".join(toks[int(a)] + b" " + toks[int(b)] + b"\n" for a, b in pairs)


def write_llama_files(out_dir, name, alphabet, pairs):
    """<name>_vocab.txt, <name>_special.txt, <name>_merges.txt under out_dir -> dict of the three paths."""
    import os
    paths = {"vocab_file": os.path.join(out_dir, name + "_vocab.txt"),
             "special_file": os.path.join(out_dir, name + "_special.txt"),
             "merges_file": os.path.join(out_dir, name + "_merges.txt")}
    for key, data in (("vocab_file", llama_vocab_text(alphabet, pairs).encode("ascii")),
                      ("special_file", llama_special_text().encode("utf-8")),
                      ("merges_file", llama_merges_bytes(alphabet, pairs))):
        with open(paths[key], "wb") as f:
            f.write(data)
    return paths
