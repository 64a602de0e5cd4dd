"""Decoding special ids without a GPU: the restatement of tests/decode_special_ref.py against hand-made cases, its two
forms against each other, the round trip encode -> decode on the references alone (the oracle's encode through
tests/specials_ref.py, then the decode rule), the new symbols in header, binding and library, the Python argument checks."""
import os
import random
import re

import numpy as np
import pytest

import decode_special_ref as DS
import helpers as H
import specials_ref as S
from decode_ref import DecodeRef
from hutoken_amd import _capi
from hutoken_amd import vocab_files as vf

NEW_SYMBOLS = ["hutk_decode_special_batch_device", "hutk_decode_special_batch"]
OUT_OF_RANGE, UNDECODABLE = 3, 4


def byte_ref(prefix=None):
    """ids 0 .. 255: the bytes in GPT-2 order; 256 " a", 257 "bc", 258 " ", 259 "  x" (keys in visible form)"""
    t = vf.bytes_to_unicode()
    toks = [bytes([b]) for b in vf.byte_token_order()] + [b" a", b"bc", b" ", b"  x"]
    ents = [(vf.encode_visible(tok, t), i) for i, tok in enumerate(toks)]
    return DecodeRef(ents, vf.gpt2_special_mapping(), prefix, True), {tok: i for i, tok in enumerate(toks)}


def char_ref():
    toks = ["▁", "a", "b", "▁a", "▁▁b", "c▁", "<0x0A>", "é"]
    ents = [(tk.encode("utf-8"), i) for i, tk in enumerate(toks)]
    return DecodeRef(ents, vf.llama_special_mapping(), "▁", False), {tk: i for i, tk in enumerate(toks)}


def both(ref, ids, specials, skip):
    """the document form, checked against the packed form on the way"""
    out, st = DS.decode_doc(ref, ids, specials, skip)
    raw, oo = DS.decode_packed(ref, ids, [0, len(ids)], specials, skip)
    assert st == 0 and raw.tobytes() == out and oo.tolist() == [0, len(out)]
    assert not DS.status(ref, ids, [0, len(ids)], specials).any()
    return out


def test_byte_vocabulary_by_hand():
    ref, t = byte_ref()
    sp = [(b"<|e|>", 1000), (b"<|s|>", 1001)]
    a, bc, sa = t[b"a"], t[b"bc"], t[b" a"]
    assert both(ref, [1000, a, bc], sp, False) == b"<|e|>abc"            # first
    assert both(ref, [a, bc, 1000], sp, False) == b"abc<|e|>"            # last
    assert both(ref, [a, 1000, 1000, 1001, bc], sp, False) == b"a<|e|><|e|><|s|>bc"  # twice in a row
    assert both(ref, [1001], sp, False) == b"<|s|>"                      # alone
    assert both(ref, [], sp, False) == b"" and both(ref, [], sp, True) == b""
    assert both(ref, [a, 1000, sa, 1001], sp, False) == b"a<|e|> a<|s|>"  # no prefix: nothing is stripped
    for ids in ([1000, a, bc], [a, 1000, 1000, 1001, bc], [a, bc, 1000]):
        assert both(ref, ids, sp, True) == b"abc"
    assert both(ref, [1001, 1000], sp, True) == b""


def test_prefix_vocabularies_by_hand():
    ref, t = char_ref()
    sp = [("<s>".encode(), 100), ("</s>".encode(), 101)]
    a, b, pa, ppb, cp, p = t["a"], t["b"], t["▁a"], t["▁▁b"], t["c▁"], t["▁"]
    # a token that begins with the prefix straight behind a special: stripped with flags 0, kept (a separator) with skip
    assert both(ref, [pa, 100, pa], sp, False) == b"a<s>a"
    assert both(ref, [pa, 100, pa], sp, True) == b"a a"
    assert both(ref, [100, pa, b], sp, False) == b"<s>ab"                # special first: the run behind it is a document
    assert both(ref, [100, pa, b], sp, True) == b"ab"                    # ... deleted: the document's front moves on
    assert both(ref, [100, 101, ppb], sp, False) == b"<s></s> b"         # one prefix off, not two
    assert both(ref, [100, 101, ppb], sp, True) == b" b"
    assert both(ref, [pa, 100, a, pa], sp, False) == b"a<s>a a"          # only the run's FIRST token loses it
    assert both(ref, [cp, 100], sp, False) == b"c <s>"
    assert both(ref, [pa, 100], sp, False) == b"a<s>" and both(ref, [100], sp, False) == b"<s>"
    assert both(ref, [p, 100, p, p], sp, False) == b"<s> "               # the prefix alone: nothing left of the first
    assert both(ref, [p, 100, p, p], sp, True) == b"  "
    # the bytes of a special are written as installed: no special-character mapping in character mode
    raw = [("▁<0x0A>".encode(), 100)]
    assert both(ref, [a, 100, pa], raw, False) == b"a" + "▁<0x0A>".encode() + b"a"
    assert both(ref, [t["<0x0A>"], pa], raw, False) == b"\n a"
    # byte mode with a prefix
    bref, bt = byte_ref(prefix="Ġ")
    sa, sp_, x = bt[b" a"], bt[b" "], bt[b"  x"]
    e = [(b"<|e|>", 5000)]
    assert both(bref, [sa, 5000, sa, sa], e, False) == b"a<|e|>a a"
    assert both(bref, [sa, 5000, sa, sa], e, True) == b"a a a"
    assert both(bref, [5000, x, 5000, sp_], e, False) == b"<|e|> x<|e|>"
    assert both(bref, [5000, x, 5000, sp_], e, True) == b" x "


def test_id_classes_by_hand():
    ref, t = byte_ref()
    a, bc = t[b"a"], t[b"bc"]
    # an id that is a vocabulary line AND special: the special wins
    assert both(ref, [a, bc, a], [(b"<bc>", bc)], False) == b"a<bc>a"
    assert both(ref, [a, bc, a], [(b"<bc>", bc)], True) == b"aa"
    # two strings with one id: the first pair's
    two = [(b"<one>", 700), (b"<two>", 700), (b"<x>", 701)]
    assert DS.strings(two) == {700: b"<one>", 701: b"<x>"}
    assert both(ref, [700, a, 701], two, False) == b"<one>a<x>"
    # ids that are neither: out of range, just above the vocabulary included; the other documents are exact
    sp = [(b"<|e|>", 1000)]
    for bad in (ref.n, ref.n + 1, 999, 1001, -1, 2**31 - 1):
        assert DS.decode_doc(ref, [a, bad, 1000], sp) == (b"", OUT_OF_RANGE)
        ids, offs = [a, 1000, a, bad, 1000, bc], [0, 2, 5, 6]
        assert DS.status(ref, ids, offs, sp).tolist() == [0, OUT_OF_RANGE, 0]
        for skip, want in ((False, [b"a<|e|>", b"a<|e|>", b"bc"]), (True, [b"a", b"a", b"bc"])):
            raw, oo = DS.decode_packed(ref, ids, offs, sp, skip)
            assert [raw.tobytes()[oo[i]:oo[i + 1]] for i in range(3)] == want
    # an undecodable vocabulary line: bad as an ordinary id, fine as a special one
    ents, special = H.random_byte_vocab(8, n_merges=100, dup_ids=True)
    dref = DecodeRef(ents, special, None, True)
    dup = int(np.nonzero(dref.bad)[0][0])
    assert DS.decode_doc(dref, [0, dup], sp) == (b"", UNDECODABLE)
    assert DS.status(dref, [0, dup], [0, 2], sp).tolist() == [UNDECODABLE]
    assert both(dref, [0, dup, 0], [(b"<dup>", dup)], False) == b"!<dup>!"


def _random_docs(rng, ref, special_ids, n_docs):
    good = [i for i in range(ref.n) if not ref.bad[i] and i not in special_ids]
    docs = []
    for _ in range(n_docs):
        docs.append([rng.choice(special_ids) if rng.random() < 0.2 else rng.choice(good)
                     for _ in range(rng.choice([0, 0, 1, 2, 3, 5, 8, 13, 30]))])
    return docs


@pytest.mark.parametrize("kind", ["byte", "bytepfx", "char"])
def test_document_form_equals_packed_form(kind):
    """1,500 random documents: the definition a document at a time against the batch form the GPU tests compare with."""
    rng = random.Random(21)
    if kind == "char":
        ents, special = H.random_char_vocab(4)
        ref = DecodeRef(ents, special, "▁", False)
    else:
        ents, special = H.random_byte_vocab(3, n_merges=300)
        ref = DecodeRef(ents, special, "Ġ" if kind == "bytepfx" else None, True)
    specials = [(b"<|endoftext|>", ref.n), (b"<|a|>", ref.n + 7), (b"<|again|>", ref.n), (b"x" * 255, 2**31 - 1),
                (b"!", 300)]  # (300: a vocabulary line as well)
    docs = _random_docs(rng, ref, [ref.n, ref.n + 7, 2**31 - 1, 300], 1500)
    offs = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    flat = np.asarray([i for d in docs for i in d], dtype=np.int64)
    assert not DS.status(ref, flat, offs, specials).any()
    for skip in (False, True):
        raw, oo = DS.decode_packed(ref, flat, offs, specials, skip)
        raw = raw.tobytes()
        for d, doc in enumerate(docs):
            assert (raw[oo[d]:oo[d + 1]], 0) == DS.decode_doc(ref, doc, specials, skip), (kind, skip, d, doc)
    plain, poo = ref.decode_packed(flat[:0], [0, 0, 0])
    raw, oo = DS.decode_packed(ref, [], [0, 0, 0], specials)
    assert len(raw) == 0 and oo.tolist() == poo.tolist() == [0, 0, 0]


def test_no_specials_is_the_plain_reference():
    ref, t = char_ref()
    ids, offs = [t["▁a"], t["b"], t["▁a"], t["▁▁b"]], [0, 2, 2, 4]
    want, want_oo = ref.decode_packed(ids, offs)
    for skip in (False, True):
        raw, oo = DS.decode_packed(ref, ids, offs, [], skip)
        assert np.array_equal(raw, want) and np.array_equal(oo, want_oo)


def test_header_binding_and_library_agree_on_the_new_symbols():
    lib = _capi.load()
    header = open(os.path.join(H.ROOT, "include", "hutoken_amd.h")).read()
    declared = set(re.findall(r"\b(hutk_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.EXPORTS, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert re.search(r"#define\s+HUTK_DECODE_SKIP_SPECIAL\s+1\b", header) and _capi.DECODE_SKIP_SPECIAL == 1
    for method in ("decode_special_packed", "decode_special_device"):
        assert hasattr(_capi.Context, method), method
    import hutoken_amd
    for name in ("decode_special", "batch_decode_special", "decode_packed_device"):
        assert name in hutoken_amd.__all__ and callable(getattr(hutoken_amd, name)), name


def test_a_host_only_context_builds_the_tables_and_refuses_the_call(vg_files, vl_files):
    for files in (vg_files, vl_files):
        vp, sp, kw = files
        ctx = _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"], device=-2)
        ctx.set_special_tokens([(b"<|endoftext|>", 50256), (b"<|im_start|>", 50257), (b"<|again|>", 50256),
                                (b"y" * 255, 2**31 - 1)])
        assert ctx.special_token_count == 4
        ids, offs = np.array([1, 50256], dtype=np.int32), np.array([0, 2], dtype=np.int64)
        with pytest.raises(RuntimeError, match="host-only"):
            ctx.decode_special_packed(ids, offs)
        oo = np.zeros(2, dtype=np.int64)
        rc = _capi.load().hutk_decode_special_batch(ctx.handle, ids.ctypes.data, offs.ctypes.data, 1, 2, None, 0,
                                                    oo.ctypes.data, None)
        assert rc == _capi.E_ARG  # an unknown flag bit is refused first
        with pytest.raises(ValueError, match="1024"):
            ctx.set_special_tokens([(b"<%d>" % i, i) for i in range(1025)])
        assert ctx.special_token_count == 4
        ctx.set_special_tokens([])
        assert ctx.special_token_count == 0
        ctx.close()
    assert _capi.load().hutk_decode_special_batch(None, None, None, 0, 0, None, 0, None, None) == _capi.E_ARG
    assert _capi.load().hutk_decode_special_batch_device(None, None, None, 0, 0, 0, None, 0, None, None, None, None) == _capi.E_ARG


def test_python_argument_checks_come_first():
    """The argument errors of decode / batch_decode (and of the tensor checks) whatever the state of the context."""
    import hutoken_amd
    for bad in (5, "12", (1, 2), None):
        with pytest.raises(RuntimeError, match="list of integers"):
            hutoken_amd.decode_special(bad)
        with pytest.raises(RuntimeError, match="single list of tokens"):
            hutoken_amd.batch_decode_special(bad)
    for fn in (hutoken_amd.decode_special, hutoken_amd.batch_decode_special):
        with pytest.raises(TypeError, match="skip_special_tokens"):
            fn([1], skip_special_tokens="yes")
    with pytest.raises(ValueError, match="special=True"):
        hutoken_amd.decode_packed_device(None, None, special=False, skip_special_tokens=True)
    with pytest.raises(TypeError, match="skip_special_tokens"):
        hutoken_amd.decode_packed_device(None, None, special=True, skip_special_tokens=None)
    with pytest.raises(TypeError, match="torch tensor"):
        hutoken_amd.decode_packed_device([1, 2], [0, 2])
    torch = pytest.importorskip("torch")
    ids, offs = torch.zeros(4, dtype=torch.int32), torch.tensor([0, 4], dtype=torch.int64)
    with pytest.raises(TypeError, match="int32"):
        hutoken_amd.decode_packed_device(ids.long(), offs)
    with pytest.raises(ValueError, match="on the GPU"):
        hutoken_amd.decode_packed_device(ids, offs, special=True)


# ---- the round trip on the references alone ----------------------------------------------------------------------------
MARKERS = ["<|endoftext|>", "<|im_start|>", "<|im_end|>"]


def _key_text(rng, ref):
    """text drawn from the vocabulary's own decoded keys (character vocabularies lack random_text's punctuation)"""
    keys = [k for k in ref.keys if k is not None and not k.startswith("<0x")]
    words = []
    for _ in range(rng.randint(0, 6)):
        w = "".join(rng.choice(keys) for _ in range(rng.randint(1, 3))).replace("▁", " ").strip()
        if w:
            words.append(w)
    return " ".join(words)


def _round_trip(oracle_mod, tmp, name, ents, special, prefix, is_byte, text_of, least):
    vp, sp = H.write_vocab(tmp, name, ents, special)
    orc = oracle_mod.Oracle(vp, sp, prefix, is_byte)
    ref = DecodeRef(ents, special, prefix, is_byte)
    rng = random.Random(7)
    specials = {MARKERS[0].encode(): ref.n + 3, MARKERS[1].encode(): ref.n, MARKERS[2].encode(): 2**31 - 1}
    docs = []
    for _ in range(400):
        pieces = [text_of(rng) for _ in range(rng.randint(1, 4))]
        docs.append((pieces, [rng.choice(MARKERS) for _ in pieces[1:]]))
    # which text pieces round-trip under the plain references
    flat = sorted({p for pieces, _m in docs for p in pieces})
    d, o = oracle_mod.pack(flat)
    ids, oo, _st = orc.encode_packed(d, o)
    ok = {}
    for i, p in enumerate(flat):
        mine = ids[int(oo[i]):int(oo[i + 1])].tolist()
        ok[p] = -1 not in mine and ref.decode_doc(mine) == (p.encode("utf-8"), 0)
    kept = [(pieces, marks) for pieces, marks in docs if all(ok[p] for p in pieces)]
    assert len(kept) >= least, "%s: the generator keeps only %d of 400 documents" % (name, len(kept))
    texts = ["".join(p + m for p, m in zip(pieces, marks + [""])) for pieces, marks in kept]
    assert any(marks for _p, marks in kept)
    d, o = oracle_mod.pack(texts)
    ids, oo, st, matches = S.encode(orc, d, o, specials)
    assert not st.any() and matches == sum(len(m) for _p, m in kept)
    raw, out_oo = DS.decode_packed(ref, ids, oo, list(specials.items()))
    assert not DS.status(ref, ids, oo, list(specials.items())).any()
    raw = raw.tobytes()
    for i, text in enumerate(texts):
        assert raw[out_oo[i]:out_oo[i + 1]] == text.encode("utf-8"), (name, i, text)
    raw, out_oo = DS.decode_packed(ref, ids, oo, list(specials.items()), skip=True)
    raw = raw.tobytes()
    if prefix is None:  # without a prefix the deleted markers leave the pieces end to end
        for i, (pieces, _m) in enumerate(kept):
            assert raw[out_oo[i]:out_oo[i + 1]] == "".join(pieces).encode("utf-8"), (name, i)
    return len(kept)


def test_round_trip_byte_vocabulary(oracle_mod, tmp_path):
    ents, special = H.random_byte_vocab(3, n_merges=500)
    kept = _round_trip(oracle_mod, tmp_path, "b", ents, special, None, True, lambda rng: H.random_text(rng), 400)
    assert kept == 400  # none is left out


def test_round_trip_byte_vocabulary_with_a_prefix(oracle_mod, tmp_path):
    ents, special = H.random_byte_vocab(5, n_merges=300)
    _round_trip(oracle_mod, tmp_path, "p", ents, special, "Ġ", True, lambda rng: H.random_text(rng), 150)


@pytest.mark.parametrize("seed", [4, 9])
def test_round_trip_character_vocabularies(oracle_mod, tmp_path, seed):
    ents, special = H.random_char_vocab(seed)
    ref = DecodeRef(ents, special, "▁", False)
    _round_trip(oracle_mod, tmp_path, "c%d" % seed, ents, special, "▁", False, lambda rng: _key_text(rng, ref), 150)
