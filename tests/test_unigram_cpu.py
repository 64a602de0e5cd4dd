"""Unigram without a GPU: (a) the restatement tests/unigram_ref.py on the hand-worked cases of the rule and on the goldens
that `tokenizers` wrote, (b) the capacity bound n_bytes + n_docs on every golden document and on adversarial ones, (c) the
argument checks and refusals of hutoken_amd.Unigram and hutoken_amd.hf.unigram_options that need no device, (d) the rule
as the kernels run it -- hutoken_amd/csrc/hutk_unigram.h, run chunk by chunk by tests/cpu/unigram_check.cpp under the
sanitizers -- against the restatement, id for id."""
import json
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import helpers as H
import unigram_cases as UC
import unigram_ref as R
import hutoken_amd
from hutoken_amd import hf

M = UC.META
SMALL = [("<unk>", 0.0), (M, -1.0), (M + "a", -1.5), ("a", -2.0), ("b", -2.5), (M + "b", -2.0), ("\tab", -1.0), ("ab", -3.0), ("b\tab", -2.0)]


def _words(text, **opts):
    return [w.decode("utf-8") for w in R.words(text, **opts)]


# ---- (a) the restatement ----
def test_words_of_the_three_shapes():
    assert _words("") == [] and _words("", whitespace_split=True) == []
    assert _words("a  b\tab") == [M + "a", M, M + "b\tab"]
    assert _words("a ") == [M + "a", M]
    assert _words("  ") == [M, M]
    assert _words(" a") == [M + "a"]
    assert _words(M + "a" + M + M + "b") == [M + "a", M, M + "b"]
    assert _words("a b", prepend_scheme="never") == ["a", M + "b"]
    assert _words("a b\nc") == [M + "a b\nc"]
    ws = dict(whitespace_split=True)
    assert _words("a  b\tab", **ws) == [M + "a", M + "b", M + "ab"]
    assert _words("  ", **ws) == []
    assert _words("a​b　c", **ws) == [M + "a​b", M + "c"]
    assert _words(M + "a" + M + M + "b c", **ws) == [M + "a", M, M + "b", M + "c"]
    assert _words("a" + M + "b", **ws) == [M + "a", M + "b"]
    co = dict(collapse_spaces=True)
    assert _words("a   b", **co) == [M + "a", M + "b"]
    assert _words("a " + M + M + " b\t\tc", **co) == [M + "a", M, M, M, M + "b\t\tc"]
    assert _words("   a", prepend_scheme="never", **co) == [M + "a"]


def test_pieces_worked_by_hand():
    v = R.Vocab(SMALL, 0)
    assert v.unk_score == -13.0
    assert v.encode("a") == ([2], [0])
    assert v.encode("a b") == ([2, 5], [0, 1])
    assert v.encode("ab") == ([1, 7], [0, 0])                 # "▁a" "b" and "▁" "ab" both score -4: the earlier last start wins
    assert v.encode("a  b\tab") == ([2, 1, 1, 8], [0, 1, 2, 2])  # "▁" "b\tab" and "▁b" "\tab" both score -3: likewise
    assert v.encode("ba") == ([5, 3], [0, 0])                 # -2 - 2 beats -1 - 2.5 - 2
    assert v.encode("xyz a") == ([1, 0, 2], [0, 0, 1])        # three unknowns fuse
    assert v.encode("xax") == ([1, 0, 3, 0], [0, 0, 0, 0])     # unknown, piece, unknown: not fused
    assert v.encode("x y") == ([1, 0, 1, 0], [0, 0, 1, 1])     # never across words
    tie = R.Vocab([("<unk>", 0.0), ("a", -1.0), ("aa", -2.0), ("aaa", -3.0)], 0)
    assert tie.encode("aaa", prepend_scheme="never") == ([3], [0])  # all paths score -3: the longest last piece, then again
    assert tie.encode("aaaa", prepend_scheme="never") == ([1, 3], [0, 0])
    dup = R.Vocab([("<unk>", 0.0), ("a", -9.0), ("b", -1.0), ("a", -1.0), ("ab", -1.5)], 0)
    assert dup.encode("ab", prepend_scheme="never") == ([4], [0])  # a(-1) + b(-1) = -2 loses; the later "a" is the one found
    lit = R.Vocab([("<unk>", -1.0), ("q", -1.0)], 0)
    assert lit.encode("<unk>x", prepend_scheme="never") == ([0], [0])  # the literal line counts as unknown and fuses
    assert lit.encode("q<unk>", prepend_scheme="never") == ([1, 0], [0, 0])


def test_ill_formed_bytes_are_characters_no_piece_matches():
    v = R.Vocab([("<unk>", 0.0), ("a", -1.0), ("é", -1.0), ("\udcc3", -0.5)], 0)  # (the last line is the lone byte C3)
    opts = dict(prepend_scheme="never")
    assert v.encode(b"a\xc3", **opts) == ([1, 0], [0, 0])
    assert v.encode(b"\xc3\xa9\xa9a", **opts) == ([2, 0, 1], [0, 0, 0])
    assert v.encode(b"\xc3 \xa9", **opts) == ([0, 0], [0, 1])  # (the space becomes U+2581, which is unknown too and fuses)


@pytest.mark.parametrize("shape", sorted(UC.SHAPES))
def test_goldens(shape):
    vocab, unk_id = UC.golden_vocab()
    g = UC.golden_docs()
    v = R.Vocab(vocab, unk_id)
    rec = g["shapes"][shape]
    assert rec["options"] == UC.SHAPES[shape] and len(g["texts"]) > 300
    for t, ids, wids in zip(g["texts"], rec["ids"], rec["word_ids"]):
        assert v.encode(t, **UC.SHAPES[shape]) == (ids, wids), (shape, t)


def test_golden_vocabulary_holds_the_hand_made_lines():
    vocab, unk_id = UC.golden_vocab()
    pieces = [p for p, _s in vocab]
    assert 2900 <= len(vocab) <= 3100 and pieces[unk_id] == "<unk>"
    assert pieces.count("ház") >= 2 and not any(c in pieces for c in UC.NO_SINGLE)
    assert max(len(p.encode()) for p in pieces) > 16 and "a b" in pieces and "a" + M + "b" in pieces and "b\tab" in pieces
    assert sum(1 for _p, s in vocab if s * 4 == int(s * 4)) >= 10


# ---- (b) the capacity bound ----
def _bound_holds(v, docs, **opts):
    for d in docs:
        b = R.to_bytes(d)
        ids, _w = v.encode(b, **opts)
        assert len(ids) <= R.folded_size(b, **opts) <= len(b) + 1, (d, opts)


def test_capacity_bound():
    vocab, unk_id = UC.golden_vocab()
    v = R.Vocab(vocab, unk_id)
    for shape, opts in UC.SHAPES.items():
        _bound_holds(v, UC.golden_docs()["texts"], **opts)
    singles = R.Vocab([("<unk>", 0.0)] + [(c, -1.0) for c in "ab é中" + M], 0)
    no_meta = R.Vocab([("<unk>", 0.0), ("a", -1.0)], 0)  # the prefix is an unknown of its own
    rng = random.Random(3)
    docs = ["a", "b", " ", M, "é", "\t", "a a a a", "a\ta\ta", "aaaa", "\t\t", " a", M + M] + UC.random_docs(rng, 200) + [b"\x80", b"\xc3", b"a\xe4\xb8"]
    for opts in UC.SHAPES.values():
        _bound_holds(singles, docs, **opts)
        _bound_holds(no_meta, docs, **opts)
    assert no_meta.encode("a") == ([0, 1], [0, 0]) and no_meta.encode("a", whitespace_split=True)[0] == [0, 1]


# ---- (c) refusals that need no device ----
def test_constructor_refusals():
    U = hutoken_amd.Unigram
    good = [("<unk>", 0.0), ("a", -1.0)]
    for vocab in ("abc", 5, {"a": 1.0}):
        with pytest.raises(TypeError):
            U(vocab, 0)
    for vocab in ([("a",)], ["a"], [(1, 1.0)], [("a", "x")], [("a", True)]):
        with pytest.raises(TypeError):
            U(vocab, 0)
    for vocab in ([], [("", 0.0)], [("a", float("nan"))], [("a", float("inf"))], [("a" * 257, 0.0)]):
        with pytest.raises(ValueError):
            U(vocab, 0)
    U([(M + "a" * 255, 0.0)], 0)  # (U+2581 counts as one byte)
    for unk in (None, "0", 1.0, True):
        with pytest.raises(TypeError):
            U(good, unk)
    for unk in (-1, 2):
        with pytest.raises(ValueError):
            U(good, unk)
    with pytest.raises(ValueError):
        U(good, 0, prepend_scheme="sometimes")
    with pytest.raises(ValueError):
        U(good, 0, prepend_scheme="never", whitespace_split=True)
    with pytest.raises(TypeError):
        U(good, 0, whitespace_split=1)
    with pytest.raises(TypeError):
        U(good, 0, collapse_spaces="yes")
    with pytest.raises(TypeError):
        U(good, 0, device="cuda")
    with pytest.raises(TypeError):
        U(good, 0, "never")  # (options are keyword-only)
    u = U(good + [("a", -2.0)], 0)
    assert u.vocab_size == 3 and u.token_to_id("a") == 2 and u.token_to_id("b") is None
    assert u.id_to_token(1) == "a" and u.id_to_token(3) is None and u.normalize is None
    assert "Unigram" in hutoken_amd.__all__
    for call in (lambda: u.batch_encode("a"), lambda: u.batch_encode([1]), lambda: u.encode(["a"])):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ValueError):
        u.batch_encode(["a"], normalize="NFX")
    with pytest.raises(TypeError):
        u.encode_packed_device(np.zeros(1, np.uint8), np.zeros(2, np.int64))


def test_from_file(tmp_path):
    model = {"type": "Unigram", "unk_id": 0, "vocab": [["<unk>", 0.0], [M + "a", -1.25]], "byte_fallback": False}
    for name, obj in (("model.json", model), ("tokenizer.json", {"version": "1.0", "model": model})):
        p = tmp_path / name
        p.write_text(json.dumps(obj), encoding="utf-8")
        u = hutoken_amd.Unigram.from_file(str(p), whitespace_split=True)
        assert u.vocab_size == 2 and u.token_to_id(M + "a") == 1 and u.unk_id == 0 and u.whitespace_split
    for k, bad in enumerate((dict(model, type="BPE"), dict(model, byte_fallback=True), dict(model, unk_id=None), [1, 2], {"model": {"type": "Unigram"}})):
        p = tmp_path / ("bad%d.json" % k)
        p.write_text(json.dumps(bad), encoding="utf-8")
        with pytest.raises(ValueError):
            hutoken_amd.Unigram.from_file(str(p))


class _Tok:
    def __init__(self, js):
        self.js = js

    def to_str(self):
        return json.dumps(self.js)


def test_unigram_options_refusals():
    ms = {"type": "Metaspace", "replacement": M, "prepend_scheme": "first", "split": True}
    model = {"type": "Unigram", "unk_id": 1, "vocab": [["a", -1.0], ["<unk>", 0.0]], "byte_fallback": False}
    rep = {"type": "Replace", "pattern": {"Regex": " {2,}"}, "content": " "}
    base = {"model": model, "normalizer": None, "pre_tokenizer": ms}
    vocab, opts = hf.unigram_options(_Tok(base))
    assert vocab == [("a", -1.0), ("<unk>", 0.0)]
    assert opts == dict(unk_id=1, prepend_scheme="always", whitespace_split=False, collapse_spaces=False, normalize=None)
    seq = {"type": "Sequence", "normalizers": [{"type": "NFKC"}, rep]}
    t5 = {"type": "Sequence", "pretokenizers": [{"type": "WhitespaceSplit"}, dict(ms, prepend_scheme="always")]}
    assert hf.unigram_options(_Tok(dict(base, normalizer=seq, pre_tokenizer=t5)))[1] == dict(
        unk_id=1, prepend_scheme="always", whitespace_split=True, collapse_spaces=True, normalize="NFKC")
    assert hf.unigram_options(_Tok(dict(base, pre_tokenizer=dict(ms, prepend_scheme="never"))))[1]["prepend_scheme"] == "never"

    def refused(match, **change):
        with pytest.raises(ValueError, match=match):
            hf.unigram_options(_Tok(dict(base, **change)))

    refused("BPE", model=dict(model, type="BPE"))
    refused("byte_fallback", model=dict(model, byte_fallback=True))
    refused("unk_id", model=dict(model, unk_id=None))
    refused("Whitespace", pre_tokenizer={"type": "Whitespace"})
    refused("none", pre_tokenizer=None)
    refused("Sequence\\[Metaspace, WhitespaceSplit\\]", pre_tokenizer={"type": "Sequence", "pretokenizers": [ms, {"type": "WhitespaceSplit"}]})
    refused("replacement", pre_tokenizer=dict(ms, replacement="_"))
    refused("split", pre_tokenizer=dict(ms, split=False))
    for name in ("Precompiled", "Strip", "Lowercase"):
        refused(name, normalizer={"type": name})
        refused(name, normalizer={"type": "Sequence", "normalizers": [{"type": "NFC"}, {"type": name}]})
        assert hf.unigram_options(_Tok(dict(base, normalizer={"type": name})), assume_normalized=True)[1]["normalize"] is None
    refused("Replace", normalizer=dict(rep, content="_"))
    refused("NFC", normalizer={"type": "Sequence", "normalizers": [rep, {"type": "NFC"}]})  # (the form would run behind the collapse)
    with pytest.raises(ValueError):
        hf.unigram_options(object())


# ---- (d) the header's rule, chunk by chunk ----
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("unigram"))
    exe = os.path.join(d, "unigram_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(H.ROOT, "hutoken_amd", "csrc"), "-o", exe,
                           os.path.join(H.ROOT, "tests", "cpu", "unigram_check.cpp")])
    return exe, d


_FLAGS = {"metaspace": 1, "never_collapse": 4, "whitespace_split": 3}


def run_header(checker, vocab, unk_id, docs, shape, chunk, tag, expect=None):
    """unigram_check on documents given as bytes; expect: (ids, offsets, word_ids), the restatement's by default."""
    exe, d = checker
    if expect is None:
        expect = R.Vocab(vocab, unk_id).encode_docs(docs, **UC.SHAPES[shape])
    ids, oo, wids = expect
    pb = [R.to_bytes(p) for p, _s in vocab]
    pdata, poffs = UC.pack(pb)
    data, offs = UC.pack(docs)
    case = os.path.join(d, tag + ".case")
    with open(case, "wb") as f:
        f.write(struct.pack("<8q", _FLAGS[shape], chunk, unk_id, len(pb), len(pdata), len(docs), len(data), len(ids)))
        f.write(poffs.tobytes() + np.asarray([s for _p, s in vocab], dtype="<f8").tobytes() + pdata.tobytes() + offs.tobytes() + data.tobytes())
        f.write(np.asarray(oo, dtype="<i8").tobytes() + np.asarray(ids, dtype="<i4").tobytes() + np.asarray(wids, dtype="<i4").tobytes())
    return subprocess.run([exe, case], capture_output=True, text=True)


ILL_FORMED = [b"\x80", b"a\x80b", b"\xc3", b"ab\xe4\xb8", b"\xe4\xb8", b"\xc0\xaf", b"\xe2\x96", b"\x96\x81 a", b"\xe2\x96\x81\x81", b"a\xe2",
              b"\x96\x81", b"\xc2", b"\xa0a", b"x\xf0\x9f\x98", b"\xa9 a", b"\xc3\xc3\xa9", b"a\xffb c", b"\xe2\x80", b"\x80\x80\x80\x80"]


@pytest.mark.parametrize("shape", sorted(UC.SHAPES))
@pytest.mark.parametrize("chunk", [16, 64, 4096])
def test_header_matches_the_goldens_and_the_restatement(checker, shape, chunk):
    vocab, unk_id = UC.golden_vocab()
    g = UC.golden_docs()
    rec = g["shapes"][shape]
    docs = [t.encode("utf-8") for t in g["texts"]]
    oo = [0]
    for ids in rec["ids"]:
        oo.append(oo[-1] + len(ids))
    expect = (sum(rec["ids"], []), oo, sum(rec["word_ids"], []))
    r = run_header(checker, vocab, unk_id, docs, shape, chunk, "g%s%d" % (shape, chunk), expect)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    rng = random.Random(chunk)
    docs = ILL_FORMED + [d.encode("utf-8") for d in UC.random_docs(rng, 300)] + [b"", b" ", b""]
    r = run_header(checker, vocab, unk_id, docs, shape, chunk, "r%s%d" % (shape, chunk))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]


def test_header_on_random_vocabularies_and_a_long_word(checker):
    rng = random.Random(8)
    for k in range(12):
        vocab, unk_id = UC.random_vocab(rng, grid=True)
        docs = [d.encode("utf-8") for d in UC.random_docs(rng, 60)] + ILL_FORMED
        for shape in UC.SHAPES:
            r = run_header(checker, vocab, unk_id, docs, shape, 16, "v%d%s" % (k, shape))
            assert r.returncode == 0, (vocab, (r.stdout + r.stderr)[-4000:])
    long_piece = "ab" * 128
    vocab = [("<unk>", 0.0), ("a", -1.0), ("b", -1.0), (long_piece, -100.0), (long_piece[:-1], -200.0), ("ab" * 20, -15.0)]
    docs = [(long_piece * 3 + "a").encode(), long_piece[:-1].encode(), (long_piece[1:] * 2).encode()]
    r = run_header(checker, vocab, 0, docs, "never_collapse", 64, "long")
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]


def test_header_sees_a_wrong_id_and_refuses_what_the_rule_refuses(checker):
    docs = [b"ab a"]
    ids, oo, wids = R.Vocab(SMALL, 0).encode_docs(docs)
    r = run_header(checker, SMALL, 0, docs, "metaspace", 16, "wrong", (ids[:-1] + [ids[-1] + 1], oo, wids))
    assert r.returncode == 1 and "expected" in r.stderr
    for k, (vocab, unk) in enumerate((([("a", 0.0), ("", 0.0)], 0), ([("a", 0.0)], 1), ([("a", float("nan"))], 0), ([("a" * 257, 0.0)], 0))):
        r = run_header(checker, vocab, unk, [], "metaspace", 16, "refuse%d" % k, ([], [0], []))
        assert r.returncode == 5 and "refused" in r.stderr, r.stdout + r.stderr
