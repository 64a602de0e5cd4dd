"""What the Unigram tests share: the golden vocabulary and documents, the three shapes, seeded vocabularies and texts, and
the `tokenizers` pipeline the goldens were written with."""
import gzip
import json
import os
import random

import wordpiece_cases as WC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_VOCAB = os.path.join(HERE, "golden", "unigram_vocab.json.gz")
GOLDEN_DOCS = os.path.join(HERE, "golden", "unigram_docs.json.gz")
META = "▁"
# name -> the options of hutoken_amd.Unigram (and of the restatement)
SHAPES = {"metaspace": dict(prepend_scheme="always", whitespace_split=False, collapse_spaces=False),
          "never_collapse": dict(prepend_scheme="never", whitespace_split=False, collapse_spaces=True),
          "whitespace_split": dict(prepend_scheme="always", whitespace_split=True, collapse_spaces=False)}
pack = WC.pack


def golden_vocab():
    """-> ([(piece, score)], unk_id)"""
    with gzip.open(GOLDEN_VOCAB, "rt", encoding="utf-8") as f:
        g = json.load(f)
    return [(p, s) for p, s in g["vocab"]], g["unk_id"]


def golden_docs():
    with gzip.open(GOLDEN_DOCS, "rt", encoding="utf-8") as f:
        return json.load(f)


def make_tokenizer(vocab, unk_id, prepend_scheme="always", whitespace_split=False, collapse_spaces=False):
    """The `tokenizers` pipeline of a shape."""
    import tokenizers
    from tokenizers import models, normalizers, pre_tokenizers
    tok = tokenizers.Tokenizer(models.Unigram([(p, float(s)) for p, s in vocab], unk_id, False))
    ms = pre_tokenizers.Metaspace(replacement=META, prepend_scheme=prepend_scheme, split=True)
    tok.pre_tokenizer = pre_tokenizers.Sequence([pre_tokenizers.WhitespaceSplit(), ms]) if whitespace_split else ms
    if collapse_spaces:
        tok.normalizer = normalizers.Replace(tokenizers.Regex(" {2,}"), " ")
    return tok


def corpus(n, seed):
    """seeded documents of the existing generators: accented Hungarian, CJK, ASCII, odd characters, literal U+2581"""
    rng = random.Random(seed)
    docs = WC.texts(n, seed, 0, 30)
    for _ in range(n // 3):
        docs.append("".join(rng.choice(["a", "b", "ab", "é", " ", "  ", META, "\t", "中", "文", "x", " ", "​", "q", "<unk>"])
                            for _ in range(rng.randint(0, 24))))
    return docs


HAND_MADE = [  # (piece, score): the lines the trained vocabulary lacks
    (META + "ab", -2.25), ("ab", -2.0), ("a", -1.0), ("b", -1.25), ("abab", -4.0), ("ba", -2.25), (META + "a", -1.75), (META, -0.75),
    ("elkáposztástalaníthatatlanság", -3.0),                                 # past 16 bytes
    ("megszentségteleníthetetlen", -3.5), ("megszentségteleníthetetlem", -3.25),  # differ in their last byte alone
    ("ház", -5.0), ("ház", -2.5),                                             # a duplicated line with another score
    ("b\tab", -1.5), ("a b", -0.5), ("a" + META + "b", -0.5), (META + "b" + META, -0.5),  # a tab; never matching: space, inner U+2581
]
NO_SINGLE = "qxő7"  # letters without a line of their own


def make_vocab(seed=20240612):
    """The golden vocabulary (tools/make_golden_unigram.py): about 3 000 pieces trained by UnigramTrainer on a seeded
    corpus, `<unk>` at id 0, then the hand-made lines."""
    import tokenizers
    from tokenizers import models, trainers
    tok = make_tokenizer([("<unk>", 0.0)], 0)
    tok.model = models.Unigram()
    trainer = trainers.UnigramTrainer(vocab_size=3000, special_tokens=[], unk_token="<unk>", show_progress=False)
    tok.train_from_iterator(WC.texts(3000, seed, 1, 40), trainer)
    model = json.loads(tok.to_str())["model"]
    vocab = [(p, s) for p, s in model["vocab"] if not (len(p) == 1 and p in NO_SINGLE)]
    unk_id = [p for p, _s in vocab].index("<unk>")
    assert isinstance(tokenizers.__version__, str)
    return vocab + HAND_MADE, unk_id


def random_vocab(rng, grid=True):
    """A small random vocabulary over a few characters: scores on a grid of quarters (ties occur) or random."""
    alphabet = ["a", "b", "c", "é", "中", META, "\t"]
    pieces = ["<unk>"]
    for _ in range(rng.randint(1, 40)):
        p = "".join(rng.choice(alphabet) for _ in range(rng.randint(1, 5)))
        pieces.append(p)
    rng.shuffle(pieces)
    score = (lambda: -0.25 * rng.randint(0, 24)) if grid else (lambda: -10.0 * rng.random())
    return [(p, score()) for p in pieces], pieces.index("<unk>")


def random_docs(rng, n):
    alphabet = ["a", "b", "c", "é", "中", META, "\t", " ", " ", "  ", "d", "\n", " ", "　"]
    return ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 20))) for _ in range(n)]
