"""Reference of the GPU normaliser and the case sets its CPU and GPU tests share.

The reference is the contract itself, per document:
    d.decode("utf-8", "surrogateescape") -> unicodedata.normalize(F, .) -> .encode("utf-8", "surrogateescape")
"""
import random
import unicodedata

import numpy as np

FORMS = ("NFC", "NFD", "NFKC", "NFKD")


def norm_doc(form, doc):
    return unicodedata.normalize(form, doc.decode("utf-8", "surrogateescape")).encode("utf-8", "surrogateescape")


def pack(docs):
    """list of bytes -> (uint8 array, int64 offsets[n + 1])"""
    offs = np.zeros(len(docs) + 1, dtype=np.int64)
    if docs:
        np.cumsum(np.fromiter(map(len, docs), dtype=np.int64, count=len(docs)), out=offs[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), offs


def reference(form, docs):
    """-> (bytes uint8, offsets int64[n + 1], changed uint8[n]) of the normalised batch"""
    out = [norm_doc(form, d) for d in docs]
    data, offs = pack(out)
    changed = np.fromiter((a != b for a, b in zip(docs, out)), dtype=np.uint8, count=len(docs))
    return data, offs, changed


_cache = {}


def _cached(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def scalar_docs():
    """every Unicode scalar value as a document of its own: 1 112 064 documents"""
    return _cached("scalars", lambda: [chr(c).encode("utf-8") for c in range(0x110000) if not 0xD800 <= c < 0xE000])


def wrapped_docs():
    """the same, each as a + c + U+0301"""
    return _cached("wrapped", lambda: [b"a" + d + b"\xcc\x81" for d in scalar_docs()])


def interesting_code_points():
    """code points that some form changes or that have a combining class"""
    def make():
        out = []
        for c in range(0x110000):
            if 0xD800 <= c < 0xE000:
                continue
            ch = chr(c)
            if unicodedata.combining(ch) or unicodedata.decomposition(ch) or 0xAC00 <= c < 0xD7A4 or 0x1100 <= c < 0x1200:
                out.append(c)
        return out
    return _cached("interesting", make)


def random_docs(n=20000, seed=20240611):
    """seeded random documents of 1..12 characters: interesting code points mixed 1:1 with plain starters"""
    def make():
        rng = random.Random(seed)
        hot = interesting_code_points()
        plain = [ord(x) for x in "aeouAEOU xyz019"] + [0x4E00, 0x3042, 0x0915, 0x09C7, 0x1100, 0xAC00, 0x1F600, 0x00DF]
        docs = []
        for _ in range(n):
            k = rng.randint(1, 12)
            docs.append("".join(chr(rng.choice(hot) if rng.random() < 0.5 else rng.choice(plain)) for _ in range(k)).encode("utf-8"))
        return docs
    return _cached(("random", n, seed), make)


EDGE_BYTES = bytes.fromhex("00417F80BFC0C2C3CCE0EDA0EFF0F4F5FF9F9882")


def byte_fuzz_docs(n=2000, seed=77):
    """seeded random byte strings of 0..40 bytes over the edge bytes: ill-formed sequences of every kind"""
    def make():
        rng = random.Random(seed)
        return [bytes(rng.choice(EDGE_BYTES) for _ in range(rng.randint(0, 40))) for _ in range(n)]
    return _cached(("bytes", n, seed), make)


NAMED = ["o\u030b", "a\u0323\u0301", "a\u0301\u0323", "a\u0301\u05ae", "\u212b", "\u0958", "\u09c7\u09be", "\u0f73",
         "\u1100\u1161\u11a8", "\uac00\u11a8", "\U00011099\U000110ba", "\U0001d15e", "\ufdfa", "\u00a0", "\ufb01", "\u2460"]
# what NFC makes of the first twelve, as the issue states it (the CPU test holds unicodedata to it)
NAMED_NFC = ["\u0151", "\u1ea1\u0301", "\u1ea1\u0301", "\u00e1\u05ae", "\u00c5", "\u0915\u093c", "\u09cb", "\u0f71\u0f72",
             "\uac01", "\uac01", "\U0001109a", "\U0001d157\U0001d165"]


def edge_docs(chunk):
    """every named segment s as "x" * p + s + "y" for p in chunk - len(s) - 2 .. chunk + 2 (lengths in bytes)"""
    docs = []
    for s in NAMED:
        b = s.encode("utf-8")
        for p in range(chunk - len(b) - 2, chunk + 3):
            docs.append(b"x" * p + b + b"y")
    return docs


BOUNDARY_DOCS = ["a", "\u0301", "", "\u0301\u0323", "\u1100", "\u1161", "\u11a8", "o", "\u030b"]


def boundary_batches(chunk):
    """documents that end inside would-be segments; then the same with each document boundary in turn placed exactly
    at byte `chunk` (the first document is lengthened in front)"""
    plain = [d.encode("utf-8") for d in BOUNDARY_DOCS]
    batches = [plain]
    for i in range(1, len(plain)):
        before = sum(map(len, plain[:i]))
        batches.append([b"x" * (chunk - before) + plain[0]] + plain[1:])
    return batches


def long_run(chunk, seed=5, tail=""):
    """a followed by 3 * chunk bytes of marks of seeded mixed classes (a whole chunk holds no boundary)"""
    rng = random.Random(seed)
    marks = ["\u0301", "\u0323", "\u0327", "\u0308", "\u05ae", "\u0315", "\u031b", "\u0345", "\u0334", "\u0e38", "\u302a"]
    s, n = ["a"], 0
    while n < 3 * chunk:
        m = rng.choice(marks)
        s.append(m)
        n += len(m.encode("utf-8"))
    return ("".join(s) + tail).encode("utf-8")


def long_run_docs(chunk):
    return [b"start", long_run(chunk), b"mid \xc3\xa9", long_run(chunk, 6, "\u0323"), b"", long_run(chunk, 7)]


def cut_docs(chunk):
    """a multi-byte character cut by the document's end, exactly at a chunk edge, for every cut of 2..4-byte characters"""
    docs, at = [], 0
    for full in ("\u00e9", "\u20ac", "\U0001f600"):
        b = full.encode("utf-8")
        for keep in range(1, len(b)):
            pad = (-(at + keep)) % chunk  # the cut piece ends at a multiple of the chunk size
            docs.append(b"z" * pad + b[:keep])
            docs.append(b[keep:] + b"\xcc\x81")  # the rest, ill-formed as well, with a mark behind it
            at += pad + len(b) + 2
    return docs
