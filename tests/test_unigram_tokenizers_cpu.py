"""The restatement tests/unigram_ref.py held to the `tokenizers` package, where that is installed: seeded random
vocabularies in the three shapes, with scores on a grid of quarters (equal path scores occur) and random ones, a
vocabulary whose only line is the unknown one, and hutoken_amd.hf.unigram_options on tokenizers built in memory."""
import random

import pytest

tokenizers = pytest.importorskip("tokenizers")

import unigram_cases as UC  # noqa: E402
import unigram_ref as R  # noqa: E402
import hutoken_amd  # noqa: E402
from hutoken_amd import hf  # noqa: E402


def _agree(vocab, unk_id, docs, tag):
    v = R.Vocab(vocab, unk_id)
    for shape, opts in UC.SHAPES.items():
        tok = UC.make_tokenizer(vocab, unk_id, **opts)
        for t, e in zip(docs, tok.encode_batch(docs, add_special_tokens=False)):
            assert v.encode(t, **opts) == (e.ids, e.word_ids), (tag, shape, t, vocab, unk_id)


@pytest.mark.parametrize("grid", [True, False])
def test_random_vocabularies_match_encode_batch(grid):
    rng = random.Random(41 if grid else 43)
    for k in range(60):
        vocab, unk_id = UC.random_vocab(rng, grid)
        _agree(vocab, unk_id, UC.random_docs(rng, 30), k)


def test_a_vocabulary_of_the_unknown_line_alone():
    rng = random.Random(5)
    _agree([("<unk>", -1.5)], 0, UC.random_docs(rng, 60) + ["<unk>", "a<unk>b", "<unk><unk>"], "unk alone")


def test_golden_vocabulary_on_a_fresh_corpus():
    vocab, unk_id = UC.golden_vocab()
    _agree(vocab, unk_id, UC.corpus(120, 77), "golden")


def test_unigram_options_reads_a_tokenizer():
    from tokenizers import normalizers, pre_tokenizers
    vocab, unk_id = [("<unk>", 0.0), ("▁a", -1.0), ("b", -2.0)], 0
    tok = UC.make_tokenizer(vocab, unk_id, **UC.SHAPES["whitespace_split"])
    got_vocab, got = hf.unigram_options(tok)
    assert got_vocab == vocab
    assert got == dict(unk_id=0, prepend_scheme="always", whitespace_split=True, collapse_spaces=False, normalize=None)
    tok = UC.make_tokenizer(vocab, unk_id, **UC.SHAPES["never_collapse"])
    tok.normalizer = normalizers.Sequence([normalizers.NFKC(), tok.normalizer])
    assert hf.unigram_options(tok)[1] == dict(unk_id=0, prepend_scheme="never", whitespace_split=False, collapse_spaces=True,
                                              normalize="NFKC")
    ug = hutoken_amd.Unigram.from_tokenizer(tok)
    assert ug.normalize == "NFKC" and ug.vocab_size == 3 and ug.token_to_id("b") == 2
    for bad, name in ((normalizers.Lowercase(), "Lowercase"), (normalizers.Strip(), "Strip")):
        tok.normalizer = bad
        with pytest.raises(ValueError, match=name):
            hf.unigram_options(tok)
        assert hf.unigram_options(tok, assume_normalized=True)[1]["normalize"] is None
    tok.normalizer = None
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    with pytest.raises(ValueError, match="Whitespace"):
        hf.unigram_options(tok)
    tok.pre_tokenizer = pre_tokenizers.Metaspace(replacement="_")
    with pytest.raises(ValueError, match="replacement"):
        hf.unigram_options(tok)
    bpe = tokenizers.Tokenizer(tokenizers.models.BPE())
    with pytest.raises(ValueError, match="Unigram"):
        hf.unigram_options(bpe)
    fb = tokenizers.Tokenizer(tokenizers.models.Unigram(vocab, 0, True))
    fb.pre_tokenizer = pre_tokenizers.Metaspace()
    with pytest.raises(ValueError, match="byte_fallback"):
        hf.unigram_options(fb)
