"""Writes tests/golden/wordpiece_vocab.txt.gz and tests/golden/wordpiece_docs.json.gz from the `tokenizers` package:
a small WordPiece vocabulary (tests/wordpiece_cases.py make_vocab) and, per setting (uncased, cased, lower_only), the
ids and word ids `tokenizers.Tokenizer.encode_batch` gives for a few hundred seeded documents.  The documents hold only
code points on which this interpreter's unicodedata and the Unicode tables inside `tokenizers` agree (the sweep of
tests/test_wordpiece_tokenizers_cpu.py finds the others), so the goldens do not depend on either's Unicode version.

    python tools/make_golden_wordpiece.py
"""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import wordpiece_cases as WC  # noqa: E402
import wordpiece_sweep as WS  # noqa: E402


def main():
    lines = WC.make_vocab()
    texts = WC.texts(300, 11, 0, 40) + ["", " \n\t ", "elkáposztástalaníthatatlanság megszentségteleníthetetlen megszentségteleníthetetlem",
                                         "xelkáposztástalaníthatatlanságoskodás", "ház Ház HÁZ haz", "q qq aq7 a7", "...!?", "中文abc字"]
    bad = WS.disagreeing_code_points()
    texts = [t for t in texts if not any(ord(c) in bad for c in t)]
    out = {"settings": {}, "texts": texts}
    for name, opts in WC.SETTINGS.items():
        tok = WS.make_tokenizer(lines, **opts)
        encs = tok.encode_batch(texts, add_special_tokens=False)
        out["settings"][name] = {"options": opts, "ids": [e.ids for e in encs], "word_ids": [e.word_ids for e in encs]}
    with open(WC.GOLDEN_VOCAB, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:
            g.write(("\n".join(lines) + "\n").encode("utf-8"))
    with open(WC.GOLDEN_DOCS, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:
            g.write(json.dumps(out, ensure_ascii=True).encode("ascii"))
    print("%d lines, %d documents, %d + %d bytes" % (len(lines), len(texts), os.path.getsize(WC.GOLDEN_VOCAB),
                                                     os.path.getsize(WC.GOLDEN_DOCS)))


if __name__ == "__main__":
    main()
