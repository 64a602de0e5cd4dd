"""Writes tests/golden/unigram_vocab.json.gz and tests/golden/unigram_docs.json.gz from the `tokenizers` package: a
Unigram vocabulary of about 3 000 pieces trained on a seeded corpus plus hand-made lines (tests/unigram_cases.py
make_vocab), and, per shape (metaspace, never_collapse, whitespace_split), the ids and word ids
`tokenizers.Tokenizer.encode_batch` gives for a few hundred seeded documents.  The corpus and the hand-made lines are
seeded; UnigramTrainer itself is not reproducible to the last bit (its hash maps are walked in an order that differs from
run to run, with one thread too), so a second run writes other scores and, here and there, other pieces: the two files
belong together and are committed together, and the tests read the vocabulary from the file, never from a new training.

    python tools/make_golden_unigram.py
"""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import unigram_cases as UC  # noqa: E402

HAND = ["", " ", "  ", "a  b\tab", "a ", " a", "▁a", "a▁▁b", "abab", "ababab", "q7 aq a7", "ház haz", "<unk> <unk>q", "q<unk>",
        "elkáposztástalaníthatatlanság megszentségteleníthetetlen megszentségteleníthetetlem", "中文abc字", "a b　c​d",
        "qqq a qaq", "x őő x"]


def _dump(path, obj):
    with open(path, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:
            g.write(json.dumps(obj, ensure_ascii=True).encode("ascii"))


def main():
    vocab, unk_id = UC.make_vocab()
    texts = UC.corpus(300, 13) + HAND
    out = {"shapes": {}, "texts": texts}
    for name, opts in UC.SHAPES.items():
        encs = UC.make_tokenizer(vocab, unk_id, **opts).encode_batch(texts, add_special_tokens=False)
        out["shapes"][name] = {"options": opts, "ids": [e.ids for e in encs], "word_ids": [e.word_ids for e in encs]}
    _dump(UC.GOLDEN_VOCAB, {"unk_id": unk_id, "vocab": [[p, s] for p, s in vocab]})
    _dump(UC.GOLDEN_DOCS, out)
    print("%d pieces, %d documents, %d + %d bytes" % (len(vocab), len(texts), os.path.getsize(UC.GOLDEN_VOCAB),
                                                      os.path.getsize(UC.GOLDEN_DOCS)))


if __name__ == "__main__":
    main()
