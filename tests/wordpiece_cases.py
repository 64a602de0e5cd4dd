"""What the WordPiece tests share: the golden vocabulary and documents, seeded texts, packing, and the settings."""
import gzip
import json
import os
import random

import numpy as np

import wordpiece_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_VOCAB = os.path.join(HERE, "golden", "wordpiece_vocab.txt.gz")
GOLDEN_DOCS = os.path.join(HERE, "golden", "wordpiece_docs.json.gz")
# name -> the options of BertNormalizer
SETTINGS = {"uncased": dict(lowercase=True, strip_accents=None),
            "cased": dict(lowercase=False, strip_accents=None),
            "lower_only": dict(lowercase=True, strip_accents=False)}

_LATIN = "abcdefghijklmnopqrstuvwxyzáéíóöőúüű"
_SYLL = ["ka", "to", "mi", "szé", "lő", "gy", "ny", "ár", "ví", "zs", "tű", "kö", "be", "el", "meg", "ság", "ség", "ház", "út",
         "ő", "és", "a", "i", "o", "u", "ék", "nak", "ban", "ből", "hoz", "er", "in", "th", "ing", "un", "re", "st"]
_CJK = "中文字漢語日本東京大学生"
_PUNCT = ".,;:!?-()[]\"'«»…–"
_ODD = ["\u200b", "\u00ad", "\u00a0", "\u2003", "\t", "\n", "\x0b", "\x85", "\ufffd", "\u0130", "\u03a3", "\u00df", "\u01c5",
        "\ud55c\uad6d", "e\u0301", "\u0378", "\U0001d49c", "\U0001f600", "\x00", "\ufb01", "\u212b", "\u0130\u0307", "\uf900",
        "\U00020000", "\u0301", "a\u0300\u0323", "\u3000", "\u2028", "\ue000", "\u0406\u0308"]


def golden_vocab():
    with gzip.open(GOLDEN_VOCAB, "rt", encoding="utf-8", newline="\n") as f:
        return f.read().split("\n")[:-1]


def golden_docs():
    with gzip.open(GOLDEN_DOCS, "rt", encoding="utf-8") as f:
        return json.load(f)


def word(rng, upper=0.2):
    w = "".join(rng.choice(_SYLL) for _ in range(rng.randint(1, 5)))
    r = rng.random()
    return w.capitalize() if r < upper else w.upper() if r < upper + 0.05 else w


def text(rng, n_words, odd=0.08):
    """a document of about n_words words: pseudo-Hungarian, punctuation, CJK, digits and the odd character"""
    out = []
    for _ in range(n_words):
        r = rng.random()
        if r < odd:
            out.append(rng.choice(_ODD))
        elif r < odd + 0.08:
            out.append(rng.choice(_PUNCT))
        elif r < odd + 0.14:
            out.append("".join(rng.choice(_CJK) for _ in range(rng.randint(1, 3))))
        elif r < odd + 0.18:
            out.append(str(rng.randint(0, 99999)))
        else:
            out.append(word(rng))
        if rng.random() < 0.8:
            out.append(rng.choice([" ", " ", " ", "  ", "\n"]))
    return "".join(out)


def texts(n, seed, lo=0, hi=40):
    rng = random.Random(seed)
    return [text(rng, rng.randint(lo, hi)) for _ in range(n)]


def make_vocab(seed=20240611):
    """The golden vocabulary (tools/make_golden_wordpiece.py writes it): specials, single characters with and without
    the prefix -- "##" forms missing for some letters --, syllable words, pieces longer than 16 bytes, pieces that are
    prefixes of other pieces, accented Hungarian and CJK characters, and one duplicated line."""
    rng = random.Random(seed)
    lines = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    chars = list(_LATIN) + list(_LATIN.upper()) + list("0123456789") + list(_CJK[:9]) + list(_PUNCT) + ["\u1112", "\u1161", "\u11ab", "i\u0307", "\u03c3", "\u00df"]
    lines += chars
    lines += ["##" + c for c in _LATIN + _LATIN.upper() + "0123456789" if c not in "qxőQXŐ7"]
    seen = set(lines)
    while len(lines) < 3000:
        w = word(rng, upper=0.15)
        for cand in (w, "##" + w, w[:max(1, len(w) // 2)], "##" + w[len(w) // 2:]):
            if cand not in seen and cand != "##":
                seen.add(cand)
                lines.append(cand)
    lines += ["elkáposztástalaníthatatlanság", "##káposztástalaníthatatlanságoskodás", "megszentségteleníthetetlen",
              "megszentségteleníthetetlem", "##megszentségteleníthetetlenségeskedéseitekért"]
    lines += [t for t in ("ház", "haz") if t not in seen]
    lines.append("ház")  # (a second time: the later id wins)
    assert lines.count("ház") == 2 and len(set(lines)) == len(lines) - 1
    return lines


def pack(docs):
    """list of bytes -> (uint8 array, int64 offsets)"""
    offs = np.zeros(len(docs) + 1, dtype=np.int64)
    if docs:
        np.cumsum([len(d) for d in docs], out=offs[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8).copy(), offs


def encode_docs(vocab, docs, **flags):
    """the restatement over documents given as bytes -> (ids, offsets, word_ids) as lists"""
    return R.encode_batch(vocab, [R.text_of(d) for d in docs], **flags)
