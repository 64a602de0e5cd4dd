"""hf.pretokenizer_preset / export()["pretokenizer"]: which split preset a tokenizer's pre-tokenizer is, on `tokenizers`
objects built in memory."""
import pytest

import importlib

from hutoken_amd import hf

PT = importlib.import_module("hutoken_amd.pretokenize")  # (the module: the package's `pretokenize` is a function)


class _Tok:
    """What hf looks at: a tokenizer whose backend is a `tokenizers.Tokenizer`."""

    def __init__(self, backend):
        self.backend_tokenizer = backend


def _with(pre):
    tokenizers = pytest.importorskip("tokenizers")
    t = tokenizers.Tokenizer(tokenizers.models.BPE())
    if pre is not None:
        t.pre_tokenizer = pre
    return _Tok(t)


def test_the_three_shapes_and_an_unknown_pattern():
    tokenizers = pytest.importorskip("tokenizers")
    from tokenizers import Regex
    from tokenizers import pre_tokenizers as P
    assert hf.pretokenizer_preset(_with(P.ByteLevel(add_prefix_space=False, use_regex=True))) == "gpt2"
    for name in ("cl100k", "qwen2"):
        split = P.Split(Regex(PT.PATTERNS[name]), "isolated")
        assert hf.pretokenizer_preset(_with(split)) == name
        # the Llama 3 / Qwen2 shape: the split, then ByteLevel as the byte map only
        seq = P.Sequence([P.Split(Regex(PT.PATTERNS[name]), "isolated"), P.ByteLevel(add_prefix_space=False, use_regex=False)])
        assert hf.pretokenizer_preset(_with(seq)) == name
    assert hf.pretokenizer_preset(_with(P.Split(Regex(r"\w+|\s+"), "isolated"))) is None
    assert hf.pretokenizer_preset(_with(P.Split(Regex(PT.PATTERNS["cl100k"] + "|x"), "isolated"))) is None
    assert hf.pretokenizer_preset(_with(P.Split(Regex(PT.PATTERNS["cl100k"]), "removed"))) is None
    assert hf.pretokenizer_preset(_with(P.ByteLevel(add_prefix_space=False, use_regex=False))) is None
    assert hf.pretokenizer_preset(_with(P.Whitespace())) is None
    assert hf.pretokenizer_preset(_with(None)) is None
    assert hf.pretokenizer_preset(object()) is None
    # two splits of the kind: neither is "the" split
    both = P.Sequence([P.Split(Regex(PT.PATTERNS["cl100k"]), "isolated"), P.ByteLevel(add_prefix_space=False, use_regex=True)])
    assert hf.pretokenizer_preset(_with(both)) is None
    assert tokenizers.__version__
