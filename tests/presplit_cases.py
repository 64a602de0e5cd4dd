"""Inputs of the pre-tokeniser tests, shared by the CPU check of the header rule and the GPU tests: the fixed alphabet,
seeded strings over it, byte strings with ill-formed UTF-8, and texts laid out around chunk, slice and bitmap-word edges.
A case is a list of documents (bytes)."""
import itertools
import random

REPRESENTATIVES = [" ", "\t", "\n", "\r", " ", "a", "s", "S", "l", "1", "'", "!", "ſ", "　"]
WHITE_SPACE = [0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000] + list(range(0x2000, 0x200B))


def _alphabet():
    a = [chr(c) for c in range(0x80)]
    a += [chr(c) for c in range(0xA0, 0x100)] + list("őűŐŰ")                    # Latin-1 and the Hungarian letters
    a += [chr(c) for c in range(0x391, 0x3CA) if c != 0x3A2] + [chr(c) for c in range(0x410, 0x450)]  # Greek, Cyrillic
    a += [chr(c) for c in range(0x4E00, 0x4E21)] + ["가"]
    a += [chr(c) for c in range(0x660, 0x66A)] + ["²"]                            # Arabic-Indic digits
    a += [chr(c) for c in WHITE_SPACE] + ["\u001c", "​", "ſ", "K", "\U0001f600"]
    return a


ALPHABET = _alphabet()
# what a text is mostly made of, so that words, contractions, digit and whitespace runs of some length occur
COMMON = list("   \n\n\t\r'''sstTrevmlLdD  ,.!?0123456789abcxyzáőж中") + [" ", "　", "ſ", "٣"]


def exhaustive(max_len=5):
    for n in range(max_len + 1):
        for t in itertools.product(REPRESENTATIVES, repeat=n):
            yield "".join(t)


def seeded(n, seed, max_chars=40):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        k = rng.randint(0, max_chars)
        src = ALPHABET if rng.random() < 0.3 else COMMON
        out.append("".join(rng.choice(src) for _ in range(k)))
    return out


def seeded_texts(n, seed, lo=20, hi=400):
    """Longer ones (documents of a batch, the fixture)."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        k = rng.randint(lo, hi)
        out.append("".join(rng.choice(ALPHABET if rng.random() < 0.15 else COMMON) for _ in range(k)))
    return out


ILL_FORMED = [b"\x80", b"\xbf\xbf", b"\xc0\xaf", b"\xc1\x81", b"\xe0\x80\x80", b"\xe0\x9f\xbf", b"\xed\xa0\x80", b"\xed\xbf\xbf",
              b"\xf0\x80\x80\x80", b"\xf0\x8f\xbf\xbf", b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xff", b"\xfe",
              b"\xc3", b"\xe2\x82", b"\xf0\x9f\x98", b"\xe2", b"\xf0\x9f", b"\xf0"]


def ill_formed(n, seed):
    """Byte strings: pieces of text, ill-formed sequences and cut characters next to one another."""
    rng = random.Random(seed)
    pieces = ILL_FORMED + [s.encode() for s in ("a", "1", " ", "\n", "'s", "!", "é", "中", "\U0001f600", "٣", "　")]
    return [b"".join(rng.choice(pieces) for _ in range(rng.randint(1, 12))) for _ in range(n)]


def _pad(n, unit="ab "):
    return (unit * (n // len(unit) + 1))[:n]


def carry_cases(chunk):
    """Texts (str, one document each) whose digit, whitespace and newline runs cross the edges of chunks of `chunk` bytes."""
    out = []
    for back in (1, 2, 3, 4, 7):  # a digit run of 3k, 3k + 1, 3k + 2 characters over one edge
        for n in (back + 1, back + 2, back + 3, 9, 10, 11):
            out.append(_pad(chunk - back) + "7" * n + "x")
            out.append(_pad(chunk - back - 1) + "!" + "7" * n)
    for n in (0, 1, 2):           # over three chunks and more, a whole chunk of digits in the middle
        out.append(_pad(chunk - 5) + "4" * (2 * chunk + 9 + n) + " a")
        out.append("9" * (3 * chunk + n))
    for back in (1, 2, 3, 5):     # two-byte digits: the count is in characters
        for n in (4, 5, 6, 7):
            out.append(_pad(chunk - back) + "٣" * n + "1" * (n % 3) + "z")
        out.append(_pad(chunk - back) + "١" * (chunk + 3 + back) + "5")
    for pre in ("a", "!", "1"):   # a whitespace run over three chunks: the last newline in the first, a middle, the last one
        for post in ("b", "", "3", "!"):
            for nl_at in (2, chunk + 7, 2 * chunk + 12, None):
                run = [" "] * (2 * chunk + 20)
                if nl_at is not None:
                    run[nl_at] = "\n"
                    run[1] = "\r"
                out.append(_pad(chunk - 11) + pre + "".join(run) + post)
    for back in (1, 2, 3):        # newline tails behind an "other" run over an edge, and over a whole chunk
        for tail in (" x", "\t\tx", "", "x", " \n y"):
            out.append(_pad(chunk - back - 1) + "?!" + "\n" * (back + 2) + tail)
            out.append(_pad(chunk - back - 1) + "a" + "\r\n" * (back + 1) + tail)
        out.append(_pad(chunk - back) + "!" + "\n" * (2 * chunk) + " \n  x")
        out.append(_pad(chunk - back) + "!" + "\n" * chunk + "\t" * chunk + "\n\t\tx")
    return out


EDGE_ITEMS = ["\U0001f600", "x's", "'ll", "a'LL", " you", " !?", "'re", "ſ't", "1234", " \n\n  a", "!\n\n b", "　　a"]


def edge_cases(edge, span=36):
    """Every item at every byte offset around a multiple of 32 bytes (a slice edge and a bitmap-word edge) near `edge`."""
    out = []
    for item in EDGE_ITEMS:
        for back in range(span):
            out.append(_pad(max(edge - back, 0), "q") + item + "z9")
    return out


def pack(docs):
    """list of bytes -> (bytes, offsets list)."""
    offs = [0]
    for d in docs:
        offs.append(offs[-1] + len(d))
    return b"".join(docs), offs
