"""The three pre-tokenisation presets (gpt2, cl100k / llama3, qwen2) restated as a sequential scanner over
`unicodedata` classes: word-start byte offsets of one document.  No regular-expression engine is used; this is the
oracle the header rule (csrc/hutk_presplit.h), the kernel and the fixtures are held to.

  gpt2    's|'t|'re|'ve|'m|'ll|'d| ?\\p{L}+| ?\\p{N}+| ?[^\\s\\p{L}\\p{N}]+|\\s+(?!\\S)|\\s+
  cl100k  (?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\\r\\n\\p{L}\\p{N}]?\\p{L}+|\\p{N}{1,3}| ?[^\\s\\p{L}\\p{N}]+[\\r\\n]*|\\s*[\\r\\n]+|\\s+(?!\\S)|\\s+
  qwen2   cl100k with \\p{N} in place of \\p{N}{1,3}

Leftmost match, first alternative that matches, greedy with backtracking.  A document is bytes; a byte that strict
UTF-8 rejects is one character that is neither letter, number nor whitespace (surrogateescape).
"""
import unicodedata

PRESETS = ("gpt2", "cl100k", "qwen2")
ALIASES = {"llama3": "cl100k"}
PATTERNS = {
    "gpt2": r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+",
    "cl100k": r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+",
    "qwen2": r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+",
}
WHITE_SPACE = frozenset([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]
                        + list(range(0x2000, 0x200B)))
assert len(WHITE_SPACE) == 25
L, N, S, O = "L", "N", "S", "O"
CONTRACTIONS = ("s", "t", "re", "ve", "m", "ll", "d")
# what each letter of a contraction matches under (?i:): itself, its capital, and for s also U+017F
FOLDS = {c: (c, c.upper()) for c in "strevmld"}
FOLDS["s"] += ("ſ",)


def char_class(ch):
    """L, N, S or O of one character (a lone surrogate = an escaped ill-formed byte: O)."""
    if ord(ch) in WHITE_SPACE:
        return S
    cat = unicodedata.category(ch)
    return L if cat[0] == "L" else N if cat[0] == "N" else O


def _contraction(s, i, fold):
    if s[i] != "'":
        return 0
    for c in CONTRACTIONS:
        t = s[i + 1:i + 1 + len(c)]
        if len(t) == len(c) and all((x in FOLDS[y]) if fold else x == y for x, y in zip(t, c)):
            return 1 + len(c)
    return 0


def _run(cls, i, what):
    while i < len(cls) and cls[i] in what:
        i += 1
    return i


def split_str(s, preset):
    """Match ends in characters: [e1, e2, ..], the last is len(s).  s: str (surrogateescape for ill-formed bytes)."""
    preset = ALIASES.get(preset, preset)
    if preset not in PRESETS:
        raise ValueError("unknown preset %r" % (preset,))
    cls = [char_class(c) for c in s]
    n = len(s)
    nl = [c in "\r\n" for c in s]
    out = []
    i = 0
    while i < n:
        e = i + _contraction(s, i, preset != "gpt2")
        if e == i and preset == "gpt2":
            j = i + 1 if s[i] == " " and i + 1 < n else i
            if cls[j] != S:
                e = _run(cls, j, cls[j])
        elif e == i:
            j = i + 1 if not nl[i] and cls[i] in (S, O) and i + 1 < n else i
            if cls[j] == L:
                e = _run(cls, j, L)
            elif cls[i] == N:
                e = i + 1 if preset == "qwen2" else min(_run(cls, i, N), i + 3)
            else:
                j = i + 1 if s[i] == " " and i + 1 < n else i
                if cls[j] == O:
                    e = _run(cls, j, O)
                    while e < n and nl[e]:
                        e += 1
        if e == i:  # whitespace
            r = _run(cls, i, S)
            last_nl = max([k for k in range(i, r) if nl[k]], default=-1)
            if preset != "gpt2" and last_nl >= 0:
                e = last_nl + 1                       # \s*[\r\n]+
            elif r == n or r - i == 1:
                e = r                                 # \s+(?!\S) up to the end, or \s+ of one character
            else:
                e = r - 1                             # \s+(?!\S): the last one is left to what follows
        out.append(e)
        i = e
    return out


def word_starts(doc, preset):
    """Byte offsets of the word starts of one document (bytes), ascending; [] for an empty document."""
    s = bytes(doc).decode("utf-8", "surrogateescape")
    at = [0]
    for c in s:
        at.append(at[-1] + len(c.encode("utf-8", "surrogateescape")))
    return [0] + [at[e] for e in split_str(s, preset)[:-1]] if s else []


def words(text, preset):
    """The pieces of a str, what pre_tokenize_str gives elsewhere."""
    ends = split_str(text, preset)
    return [text[a:b] for a, b in zip([0] + ends[:-1], ends)]
