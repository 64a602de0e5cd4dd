"""The restatement (wordpiece_ref.py) against the `tokenizers` package, code point by code point.  Imported only where
`tokenizers` is installed (test_wordpiece_tokenizers_cpu.py, tools/make_golden_wordpiece.py, tools/bench_wordpiece.py)."""
import functools

import wordpiece_ref as R


def make_tokenizer(lines, unk_token="[UNK]", prefix="##", max_input_chars_per_word=100, **options):
    """a tokenizers.Tokenizer built in memory: models.WordPiece behind BertNormalizer and BertPreTokenizer"""
    import tokenizers
    vocab = {}
    for i, t in enumerate(lines):
        vocab[t] = i  # (the later id wins, as models.WordPiece.read_file has it)
    tok = tokenizers.Tokenizer(tokenizers.models.WordPiece(vocab, unk_token=unk_token, continuing_subword_prefix=prefix,
                                                           max_input_chars_per_word=max_input_chars_per_word))
    tok.normalizer = tokenizers.normalizers.BertNormalizer(**options)
    tok.pre_tokenizer = tokenizers.pre_tokenizers.BertPreTokenizer()
    return tok


@functools.lru_cache(maxsize=None)
def sweep():
    """-> {code point: [what differs]}: the normaliser under the four lowercase x strip_accents settings, and the
    punctuation rule, over every code point but the surrogates."""
    import tokenizers
    out = {}
    scalars = [c for c in range(0x110000) if not 0xD800 <= c < 0xE000]
    for lowercase in (False, True):
        for strip in (False, True):
            theirs = tokenizers.normalizers.BertNormalizer(lowercase=lowercase, strip_accents=strip).normalize_str
            for c in scalars:
                ch = chr(c)
                if theirs(ch) != R.normalize(ch, lowercase=lowercase, strip_accents=strip):
                    out.setdefault(c, []).append("normaliser lowercase=%s strip_accents=%s" % (lowercase, strip))
    split = tokenizers.pre_tokenizers.BertPreTokenizer().pre_tokenize_str
    for c in scalars:
        s = "a%sa" % chr(c)
        if [p for p, _span in split(s)] != R.split(s):
            out.setdefault(c, []).append("split")
    return out


def disagreeing_code_points():
    return frozenset(sweep())
