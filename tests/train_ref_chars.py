"""A pure-Python restatement of the trainer's "chars" mode (tools/train_vocab.cpp ... chars), for the tests.

  1 words      as in bytes mode: train_ref.word_counts
  2 skip       a unique word holding a byte < 0x20 or 0x7F is dropped (its characters do not enter the alphabet)
  3 space      in every kept word, ' ' becomes E2 96 81 (U+2581), before the word is cut
  4 characters cut left to right, the length from the lead byte: < 0x80 1, 110xxxxx 2, 1110xxxx 3, anything else 4
               (stray continuation bytes and F0..FF included); a character is cut short at the word's end
  5 alphabet   the distinct characters, sorted as byte strings, are the symbols 0..A-1
  6 merges     bytes mode's loop (train_ref.train_words), merge k creating symbol A + k"""
import helpers
import train_ref

SPACE = b"\xe2\x96\x81"


def char_len(lead):
    return 1 if lead < 0x80 else 2 if lead & 0xE0 == 0xC0 else 3 if lead & 0xF0 == 0xE0 else 4


def split_chars(word):
    """The characters of one kept word (rules 3 and 4)."""
    s = word.replace(b" ", SPACE)
    out, i = [], 0
    while i < len(s):
        n = char_len(s[i])
        out.append(s[i:i + n])
        i += n
    return out


def dropped(word):
    return any(c < 0x20 or c == 0x7F for c in word)


def symbolise(counts):
    """{word bytes: count} -> (alphabet [bytes], {tuple of symbol ids: count}, number of dropped unique words)."""
    kept = {w: c for w, c in counts.items() if not dropped(w)}
    cut = {w: split_chars(w) for w in kept}
    alphabet = sorted({ch for chars in cut.values() for ch in chars})
    ids = {ch: i for i, ch in enumerate(alphabet)}
    words = {}
    for w, chars in cut.items():
        key = tuple(ids[ch] for ch in chars)
        words[key] = words.get(key, 0) + kept[w]
    return alphabet, words, len(counts) - len(kept)


def train_words(counts, n_merges):
    """{word bytes: count} -> (alphabet, pairs [(a, b)], pair counts [int], dropped)."""
    alphabet, words, n_dropped = symbolise(counts)
    A = len(alphabet)
    # train_ref.train_words numbers merge k as 256 + k.  Its input symbols are shifted to -A..-1 so that they stay
    # below every merge symbol: the map (char i -> i - A, symbol A + k -> 256 + k) keeps the order of every pair, so
    # the selection (ties to the smaller pair) is unchanged, and mapping the pairs back gives the chars-mode answer.
    shifted = {tuple(x - A for x in w): c for w, c in words.items()}
    pairs, cnts = train_ref.train_words(shifted, n_merges)
    back = lambda x: x + A if x < 0 else x - 256 + A  # noqa: E731
    return alphabet, [(back(a), back(b)) for a, b in pairs], cnts, n_dropped


def train(docs, n_merges):
    return train_words(train_ref.word_counts(docs), n_merges)


def tokens(alphabet, pairs):
    """Byte strings of every symbol: the alphabet, then one per merge."""
    toks = list(alphabet)
    for a, b in pairs:
        toks.append(toks[a] + toks[b])
    return toks


def edge_docs(rng):
    """Lines that reach every rule: invalid UTF-8 next to spaces, literal U+2581, 4-byte characters, bytes 80..BF and
    F8..FF, lead bytes at a word's end, and words with control bytes whose characters appear nowhere else."""
    pool = [b"a", b"b", b" ", b"  ", b"\xe2\x96\x81", b"\xe2", b"\xe2\x96", b"\xf0\x9f\x98\x82", b"\xf0\x9f",
            b"\xf0ab", b"\x80", b"\xbf", b"\x9f", b"\xf8", b"\xfc", b"\xff", b"\xc3\xa9", b"\xc3", b"\xe6\xbc\xa2",
            b"x", b"y", b".", b"1", b"\xc0\xa0", b"\xed\xa0\x80", b"\xf4\x90\x80\x80"]
    docs = []
    for _ in range(400):
        r = rng.random()
        if r < 0.45:
            d = b"".join(rng.choice(pool) for _ in range(rng.randint(1, 30)))
        elif r < 0.7:
            d = helpers.random_text(rng, max_words=15, exotic=0.6).encode("utf-8")
        elif r < 0.85:
            d = helpers.random_bytes_text(rng, rng.randint(1, 40))
        else:  # control bytes around characters seen nowhere else (they must not enter the alphabet)
            d = (b"q" + bytes([rng.choice([0x01, 0x1F, 0x7F])]) + b"\xea\x80\x80 " + bytes([rng.choice([0x01, 0x7F])]) +
                 b"\xe1\x9a\xa0 z" + rng.choice([b"\xd0\x96", b"\xf0\x90\x8d\x88", b""]) + b"\x7f")
        docs.append(d.replace(b"\n", b" ").replace(b"\r", b" "))
    return docs
