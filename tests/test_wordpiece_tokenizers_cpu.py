"""The restatement tests/wordpiece_ref.py held to the `tokenizers` package, where that is installed: (a) the sweep over
every code point -- normaliser under the four lowercase x strip_accents settings, and the punctuation rule --, whose
disagreements are the difference between this interpreter's Unicode tables and the ones inside `tokenizers`, (b) the
whole pipeline against tokenizers.Tokenizer.encode_batch on a seeded corpus drawn from outside that set, (c)
WordPiece.from_tokenizer on tokenizers built in memory, and its refusals."""
import random
import unicodedata

import pytest

tokenizers = pytest.importorskip("tokenizers")

import wordpiece_cases as WC  # noqa: E402
import wordpiece_ref as R  # noqa: E402
import wordpiece_sweep as WS  # noqa: E402
import hutoken_amd  # noqa: E402


def test_sweep_disagreements_are_few_high_and_of_the_expected_kinds():
    """Measured with Python 3.10 (Unicode 13.0) against tokenizers 0.22.2: 463 code points, the lowest U+07FD."""
    sw = WS.sweep()
    print("disagreeing code points: %d, lowest U+%04X, %d in the BMP" % (len(sw), min(sw) if sw else 0, sum(c < 0x10000 for c in sw)))
    assert len(sw) <= 512
    assert not sw or min(sw) >= 0x0780
    for c in sw:
        k = unicodedata.category(chr(c))
        assert k in ("Mn", "Mc", "Cf", "Cn", "So") or k.startswith("P"), (hex(c), k, sw[c])


def _corpus(n, seed):
    """seeded documents over code points on which both sides' tables agree"""
    bad = WS.disagreeing_code_points()
    rng = random.Random(seed)
    pool = [c for c in list(range(0x20, 0x250)) + list(range(0x370, 0x530)) + list(range(0x2000, 0x2070)) + list(range(0x3000, 0x3100))
            + list(range(0x4E00, 0x4E80)) + list(range(0xAC00, 0xAC40)) + [0x9, 0xA, 0xD, 0xB, 0x85, 0x0, 0xFFFD, 0xE000, 0x1D49C, 0x1F600,
                                                                          0x2B820, 0x2B920, 0xF900, 0x300, 0x301, 0x323, 0x1E9E, 0x130]
            if c not in bad]
    docs = [t for t in WC.texts(n, seed, 0, 40) if not any(ord(c) in bad for c in t)]
    for _ in range(n // 2):
        docs.append("".join(chr(rng.choice(pool)) if rng.random() < 0.5 else rng.choice("abé ,") for _ in range(rng.randint(0, 60))))
    return docs


@pytest.mark.parametrize("setting", sorted(WC.SETTINGS))
def test_pipeline_matches_encode_batch(setting):
    lines = WC.golden_vocab()
    opts = WC.SETTINGS[setting]
    tok = WS.make_tokenizer(lines, **opts)
    docs = _corpus(400, 97)
    v = R.Vocab(lines)
    for t, e in zip(docs, tok.encode_batch(docs, add_special_tokens=False)):
        assert R.encode(v, t, **opts) == (e.ids, e.word_ids), (setting, t)


def test_pipeline_matches_with_other_options():
    lines = WC.golden_vocab()
    docs = _corpus(150, 5)
    for opts in (dict(clean_text=False), dict(handle_chinese_chars=False), dict(lowercase=False, strip_accents=True)):
        for max_chars in (1, 4, 100):
            tok = WS.make_tokenizer(lines, max_input_chars_per_word=max_chars, **opts)
            v = R.Vocab(lines, max_input_chars_per_word=max_chars)
            for t, e in zip(docs, tok.encode_batch(docs, add_special_tokens=False)):
                assert R.encode(v, t, **opts) == (e.ids, e.word_ids), (opts, max_chars, t)
    tok = WS.make_tokenizer(["a", "b", "a", "@@a"], unk_token="b", prefix="@@")
    v = R.Vocab(["a", "b", "a", "@@a"], unk_token="b", prefix="@@")
    for t in ("a aa aaa ab", ""):
        assert R.encode(v, t) == (tok.encode(t, add_special_tokens=False).ids, tok.encode(t, add_special_tokens=False).word_ids)


def test_from_tokenizer_reads_options_and_vocabulary():
    lines = [t for i, t in enumerate(WC.golden_vocab()) if t != "ház" or i > 3000]  # (a dict holds every token once)
    tok = WS.make_tokenizer(lines, max_input_chars_per_word=7, lowercase=False, strip_accents=True, handle_chinese_chars=False)
    wp = hutoken_amd.WordPiece.from_tokenizer(tok)
    assert wp.vocab_size == len(lines) and [wp.id_to_token(i) for i in range(len(lines))] == lines
    assert wp.max_input_chars_per_word == 7 and wp.unk_token == "[UNK]" and wp.continuing_subword_prefix == "##"
    from hutoken_amd import wordpiece as WT
    assert wp._flags == WT.CLEAN_TEXT | WT.STRIP_ACCENTS
    wp = hutoken_amd.WordPiece.from_tokenizer(WS.make_tokenizer(lines))
    assert wp._flags == 15 and wp.max_input_chars_per_word == 100

    class Fast:  # what a transformers fast tokenizer looks like from here
        backend_tokenizer = tok
    assert hutoken_amd.WordPiece.from_tokenizer(Fast()).vocab_size == len(lines)


def test_from_tokenizer_refuses_anything_else():
    T = tokenizers
    lines = ["[UNK]", "a"]
    good = WS.make_tokenizer(lines)
    bpe = T.Tokenizer(T.models.BPE())
    with pytest.raises(ValueError, match="BPE"):
        hutoken_amd.WordPiece.from_tokenizer(bpe)
    t = WS.make_tokenizer(lines)
    t.normalizer = T.normalizers.NFC()
    with pytest.raises(ValueError, match="NFC"):
        hutoken_amd.WordPiece.from_tokenizer(t)
    t = WS.make_tokenizer(lines)
    t.pre_tokenizer = T.pre_tokenizers.Whitespace()
    with pytest.raises(ValueError, match="Whitespace"):
        hutoken_amd.WordPiece.from_tokenizer(t)
    t = T.Tokenizer(T.models.WordPiece({"[UNK]": 0, "a": 1}, unk_token="[UNK]"))
    with pytest.raises(ValueError, match="none"):
        hutoken_amd.WordPiece.from_tokenizer(t)
    with pytest.raises(ValueError, match="str"):
        hutoken_amd.WordPiece.from_tokenizer("bert-base-uncased")
    t = T.Tokenizer(T.models.WordPiece({"[UNK]": 0, "a": 5}, unk_token="[UNK]"))
    t.normalizer, t.pre_tokenizer = good.normalizer, good.pre_tokenizer
    with pytest.raises(ValueError, match="gaps"):
        hutoken_amd.WordPiece.from_tokenizer(t)
