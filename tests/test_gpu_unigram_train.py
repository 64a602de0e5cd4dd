"""Unigram training on the GPU (csrc/hutk_unigram_train.h) against tests/unigram_train_ref.py, layer by layer on the
same inputs: the E-step within a bound derived from its length, the M-step to 1e-12, alternatives, histogram and kept set exactly.
Needs an MI355X."""
import collections
import random

import numpy as np
import pytest

import unigram_cases as UC
import unigram_ref as R
import unigram_train_ref as T
from test_gpu_unigram import M, _dev, _to_device
from test_gpu_unigram_sample import VOCABS, _docs

pytestmark = pytest.mark.gpu
SMALL = VOCABS["small"][0]
B, AB = 3, 4  # ids of "b" and "ab" in SMALL


def _trainer(vocab, shape="metaspace", dead=()):
    import hutoken_amd as H
    tr = H.UnigramTrainer(list(vocab), 0, **UC.SHAPES[shape])
    scores = np.array([s for _p, s in vocab])
    scores[list(dead) + [0]] = np.nan
    tr.set_scores(scores)
    return tr, [p for p, _s in vocab], scores


def _close(got, want, words):
    """The E-step's bound: 16 n max(1, |Z|) 2^-53 relative plus 1e-12, n the longest word in folded bytes; for the sum of Z, summed over
    the words.  want: unigram_train_ref.e_step's four results."""
    n = max([len(w) - 2 * w.count(R.META) for w in words] + [1])
    rtol = 16 * n * max(1.0, want[2]) * 2.0 ** -53
    expected, stats = (t.cpu().numpy() for t in got)
    assert np.all(np.abs(expected - want[0]) <= rtol * want[0] + 1e-12), np.abs(expected - want[0]).max()
    assert stats[1] == want[1][1] and abs(stats[0] - want[1][0]) <= rtol * want[3] + 1e-12 * want[1][1]


@pytest.mark.parametrize("name,shape,dead,accumulator", [("small", s, (), "table") for s in sorted(UC.SHAPES)]
                         + [("small", "metaspace", (B,), "table"), ("small", "never_collapse", (AB, 12), "atomics"),
                            ("long", "metaspace", (), "table"), ("long", "never_collapse", (B,), "atomics")])
def test_e_step(name, shape, dead, accumulator):
    vocab = VOCABS[name][0]
    docs = _docs(VOCABS[name][1]) + [b"<unk> a<unk>b", b"a" * 5]
    tr, pieces, scores = _trainer(vocab, shape, dead)
    words = T.corpus_words(docs, **UC.SHAPES[shape])
    want = T.e_step(T.model(pieces, scores, 0), words, len(pieces))
    if B in dead:  # a dead single character
        full = np.array([np.nan] + [sc for _p, sc in vocab[1:]])
        assert want[0][0] > T.e_step(T.model(pieces, full, 0), words, len(pieces))[0][0]  # more unknown edges
    _close(tr.e_step(_to_device(docs), accumulator=accumulator), want, words)
    half = len(docs) // 2  # two halves of the batch, added into the same tensors
    _close(tr.e_step([_to_device(docs[:half]), _to_device(docs[half:])], accumulator=accumulator), want, words)
    empty = tr.e_step(_to_device([]))
    assert not empty[0].any() and not empty[1].any()


def test_e_step_of_a_plain_vocabulary_and_the_hot_piece():
    import hutoken_amd as H
    docs = _docs(32) + [b"<unk> a<unk>b"]  # every line is alive and the unknown line's text is a key like any other
    ug = H.Unigram(list(SMALL), 0)
    words = T.corpus_words(docs, **UC.SHAPES["metaspace"])
    want = T.e_step(R.Vocab(SMALL, 0), words, len(SMALL))
    assert want[0][0] > 1.5
    _close(ug.expected_counts_device(*_to_device(docs)), want, words)
    hot = H.Unigram(list(SMALL), 0, **UC.SHAPES["never_collapse"])  # 4096 words "a": one path each, every posterior is 1
    for accumulator in ("table", "atomics"):
        expected, stats = hot.expected_counts_device(*_to_device([b"a"] * 4096), accumulator=accumulator)
        assert expected[11].item() == 4096.0 and expected.sum().item() == 4096.0 and stats.tolist() == [4096 * SMALL[11][1], 4096.0]


def test_m_step():
    import torch
    tr, _pieces, _scores = _trainer(SMALL)
    counts = np.array([3.0, 0.4999999, 0.5, 0.0, 2.5, 1e6, 0.5000001, 0.25] + [7.0 + k for k in range(len(SMALL) - 8)])  # "b" (3): a zero
    alive = tr.m_step(torch.from_numpy(counts).to(_dev()))
    want = T.m_step(counts, 0)
    got = tr.scores
    assert alive == np.count_nonzero(~np.isnan(want)) == tr.alive and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= 1e-12 * np.abs(want[ok]))
    docs = [b"ab b\xc3\xa9"]  # the scores are the handle's: the next E-step runs on them, "b" dead, the unknown score the new minimum - 10
    words = T.corpus_words(docs, **UC.SHAPES["metaspace"])
    _close(tr.e_step(_to_device(docs)), T.e_step(T.model(_pieces, want, 0), words, len(SMALL)), words)


def _random_vocab(rng, grid):
    out = []
    while len(out) < 6:  # no duplicates, no line that can never be a key, and more than a handful of lines
        seen, out = set(), [("<unk>", 0.0)]
        for p, s in UC.random_vocab(rng, grid)[0]:
            if p != "<unk>" and p not in seen and M not in p[1:]:
                seen.add(p)
                out.append((p, s))
    return out


@pytest.mark.parametrize("case", ["small", "small_dead_b", "long"] + ["grid%d" % k for k in range(4)] + ["random%d" % k for k in range(4)])
def test_alternatives(case):
    rng = random.Random(case)
    vocab = VOCABS["long" if case == "long" else "small"][0] if not case[-1].isdigit() else _random_vocab(rng, case.startswith("grid"))
    tr, pieces, scores = _trainer(vocab, dead=(B,) if case == "small_dead_b" else ())
    want_cls, want_alts = T.alternatives(T.model(pieces, scores, 0), pieces, scores)
    if case == "small_dead_b":
        assert want_alts[AB] == [11, 0]  # "ab" without "b": "a", then the unknown edge
    if case == "long":
        assert want_cls[-1] == 3 and len(want_alts[len(pieces) - 1]) > 2  # the 256-byte piece; "a" * 8 and "a" * 9 are lines of SMALL
    cls, alts = tr.alternatives()
    assert cls.tolist() == want_cls and alts == want_alts


@pytest.mark.parametrize("case", ["small", "random1", "random2"])
def test_histogram_losses_and_the_kept_set(case):
    rng = random.Random(case)
    vocab, docs = (SMALL, _docs(32)) if case == "small" else (_random_vocab(rng, False), UC.random_docs(rng, 300))
    docs = [R.to_bytes(d) for d in docs + [p for i, (p, _s) in enumerate(vocab) for _ in range(1 + i * 7 % 5)]]  # every line a word of its own
    tr, pieces, scores = _trainer(vocab, "never_collapse")
    v, words = T.model(pieces, scores, 0), T.corpus_words(docs, **UC.SHAPES["never_collapse"])
    want_freq = T.histogram(v, words, len(pieces))
    freq = tr.histogram(_to_device(docs))
    assert freq.cpu().numpy().tolist() == want_freq.tolist()
    want = T.losses(want_freq, *T.alternatives(v, pieces, scores))
    tr.alternatives()
    loss = tr.losses(freq).cpu().numpy()
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(loss), np.isnan(want)) and np.array_equal(loss[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    assert fin.sum() >= 3 and np.all(np.abs(loss[fin] - want[fin]) <= 1e-12 * np.abs(want[fin]))
    desired = int((want == np.inf).sum()) + int(fin.sum()) // 2  # the cut falls among the candidates
    keep, gap = T.kept(want, desired)
    assert gap > 1e-6, "the reference's losses either side of the cut are too close: take another case"
    assert tr.prune(_to_device(docs), desired) == len(keep) and np.flatnonzero(~np.isnan(tr.scores)).tolist() == keep


def _fit_corpus(seed, n=300):
    """Words of one to four syllables drawn with falling weights: no two pieces get the same count, which unigram_cases.corpus' rare
    characters do (equal sums taken in another order fall either way in f64, and the lines' order with them)."""
    rng = random.Random(seed)
    syl = ["ka", "to", "ri", "men", "é", "su", "no", "中", "shi", "ba", "l", "o", "an", "te", "ku", "文", "r", "7"]
    weights = [1.0 / (k + 1) ** 0.8 for k in range(len(syl))]
    return [" ".join("".join(rng.choices(syl, weights, k=rng.randint(1, 4))) for _ in range(rng.randint(3, 14))) for _ in range(n)]


def test_fit_end_to_end():
    import hutoken_amd as H
    docs = _fit_corpus(1)
    words = [w.decode() for w in T.corpus_words(docs, **UC.SHAPES["metaspace"])]
    subs = collections.Counter(w[i:i + k] for w in words for k in range(2, 7) for i in range(len(w) - k + 1) if M not in w[i:i + k][1:])
    chars = sorted({c for w in words for c in w})
    seed = ["<unk>"] + chars + [s for s, _c in sorted(subs.items(), key=lambda t: (-t[1], t[0]))[:400]]
    vocab_size = len(chars) + 1 + 60
    start = [float(np.log(1.0 / len(seed)))] * len(seed)
    want, n_top, z_top = T.fit(seed, start, 0, docs, vocab_size, **UC.SHAPES["metaspace"])  # (asserts its margins: 0.5, the cuts, neighbours)
    tr = H.UnigramTrainer(seed)
    ug = tr.fit(_to_device([d.encode() for d in docs]), vocab_size)
    rtol = 16 * n_top * max(1.0, z_top) * 2.0 ** -53
    for got in (ug, H.train_unigram(docs, seed, vocab_size)):
        assert got._pieces == [p for p, _s in want] and got.unk_id == 0 and got.vocab_size == vocab_size
        assert all(abs(a - b) <= rtol * abs(b) + 1e-12 for a, (_p, b) in zip(got._scores, want))
    assert tr.passes >= 5 and 0 not in ug.encode_packed_device(*_to_device([d.encode() for d in docs]))[0].tolist()
