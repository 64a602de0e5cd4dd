"""The plain restatement of token spans (tests/spans_ref.py) against the CPU oracle: the definition by decoded prefixes
 on documents without -1 ids, the per-token properties on all of them, hand-written cases, and the
C symbols of the device form.  The GPU kernels are then compared with the restatement in tests/test_gpu_spans.py."""
import random

import numpy as np
import pytest

import helpers as H
import spans_ref as S

VOCABS = ["VG", "VL", "VC"]


def _oracle(oracle_mod, name):
    from hutoken_amd import data
    vp, sp, kw = data.vocab_files(name)
    return oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"]), kw["is_byte_encoder"]


def _docs(name, is_byte):
    """Short documents: corpus slices (cut at a character boundary), random texts, and for byte-encoder vocabularies
    arbitrary byte strings."""
    from hutoken_amd import synth
    out = []
    for c in ("C2", "C3", "C5"):
        d, o = synth.corpus(c, 12)
        raw = d.tobytes()
        for i in range(12):
            doc = raw[int(o[i]):int(o[i + 1])][:90]
            while doc and (doc[-1] & 0xC0) == 0x80:  # not inside a character ...
                doc = doc[:-1]
            if doc and doc[-1] >= 0xC0:  # ... and not behind its lead byte
                doc = doc[:-1]
            out.append(doc)
    rng = random.Random(len(name) * 77 + ord(name[1]))
    out += [H.random_text(rng, max_words=8).encode("utf-8") for _ in range(60)]
    if is_byte:
        out += [H.random_bytes_text(rng, rng.randint(0, 30)) for _ in range(40)]
    return out


def _check_properties(tt, doc, ids, status, is_byte):
    """What holds for every document, with or without -1 ids."""
    sp, st = S.byte_spans(tt, doc, ids, is_byte)
    assert st == 0, (doc, ids)
    bounds = set(S.item_bounds(doc, is_byte))
    at = 0
    for k, (i, (s, e)) in enumerate(zip(ids, sp)):
        assert s == at and e >= s  # the tokens tile the document from byte 0 on
        at = e
        if i == -1:
            assert s in bounds and e in bounds and e > s
            assert not any(s < b < e for b in bounds), "an id of -1 covers exactly one item"
        elif k > 0:
            assert doc[s:e] == tt.rest(i)
        else:
            assert doc[s:e] == tt.first(i)
    if status == 0:
        assert at == len(doc)
    ch = S.to_chars(doc, sp)
    text = doc.decode("utf-8", "replace")
    if doc.decode("utf-8", "ignore").encode("utf-8") == doc:  # valid UTF-8: character spans slice the str
        for (s, e), (cs, ce) in zip(sp, ch):
            if e > s and (doc[s] & 0xC0) != 0x80 and (e == len(doc) or (doc[e] & 0xC0) != 0x80):
                assert text[cs:ce].encode("utf-8") == doc[s:e]
    return sp


@pytest.mark.parametrize("name", VOCABS)
def test_definition_by_decoded_prefixes(oracle_mod, name):
    orc, is_byte = _oracle(oracle_mod, name)
    tt = S.TokenText(orc)
    with_unknown = 0
    for doc in _docs(name, is_byte):
        ids, status = orc.encode_bytes(doc)
        sp = _check_properties(tt, doc, ids, status, is_byte)
        if -1 in ids:
            with_unknown += 1
            continue
        for k in range(len(ids)):  # end_k = len(decode(ids[:k + 1])), and that prefix IS the document's
            out, st = orc.decode_bytes(ids[:k + 1])
            assert st == 0
            assert sp[k][1] == len(out) and doc[:len(out)] == out, (name, doc, ids, k)
            assert sp[k][0] == (sp[k - 1][1] if k else 0)
    if name == "VL":
        assert with_unknown > 0  # the Llama-shaped vocabulary does not hold every character of these texts


@pytest.mark.parametrize("drop", ["őű漢", "e3.", "aeiouáé字"])
def test_character_vocabulary_with_dropped_characters(tmp_path, oracle_mod, drop):
    ents, special = H.random_char_vocab(5, n_merges=400, drop_chars=drop)
    vp, spath = H.write_vocab(tmp_path, "c%d" % len(drop), ents, special)
    orc = oracle_mod.Oracle(vp, spath, "▁", False)
    tt = S.TokenText(orc)
    rng = random.Random(9)
    unknown = 0
    for _ in range(150):
        doc = H.random_text(rng, max_words=10).encode("utf-8")
        ids, status = orc.encode_bytes(doc)
        _check_properties(tt, doc, ids, status, False)
        unknown += -1 in ids
    assert unknown > 0


def test_byte_vocabulary_small(tmp_path, oracle_mod):
    ents, special = H.random_byte_vocab(3, n_merges=300)
    vp, spath = H.write_vocab(tmp_path, "b", ents, special)
    orc = oracle_mod.Oracle(vp, spath, None, True)
    tt = S.TokenText(orc)
    rng = random.Random(4)
    for k in range(200):
        doc = H.random_text(rng, max_words=10).encode("utf-8") if k % 2 else H.random_bytes_text(rng, rng.randint(0, 40))
        ids, status = orc.encode_bytes(doc)
        _check_properties(tt, doc, ids, status, True)


def test_leading_space_with_a_prefix_gives_empty_spans_first(oracle_mod):
    orc, is_byte = _oracle(oracle_mod, "VL")
    tt = S.TokenText(orc)
    doc = " hello world".encode("utf-8")
    ids, _ = orc.encode_bytes(doc)
    sp, st = S.byte_spans(tt, doc, ids, is_byte)
    assert st == 0 and sp[0] == (0, 0) and sp[1][0] == 0 and sp[-1][1] == len(doc)
    assert S.to_chars(doc, sp)[0] == (0, 0)
    plain, _ = orc.encode_bytes(b"hello world")
    sp2, st2 = S.byte_spans(tt, b"hello world", plain, is_byte)
    assert st2 == 0 and sp2[0][0] == 0 and sp2[0][1] > 0  # no leading space: the prefix is stripped from the first token


def test_a_character_split_across_byte_level_tokens_is_reported_by_both(tmp_path, oracle_mod):
    ents, special = H.random_byte_vocab(3, n_merges=300)
    vp, spath = H.write_vocab(tmp_path, "s", ents, special)
    orc = oracle_mod.Oracle(vp, spath, None, True)
    tt = S.TokenText(orc)
    found = 0
    for ch in "漢字€😂őé":
        doc = ("a" + ch + "b").encode("utf-8")
        ids, _ = orc.encode_bytes(doc)
        sp, st = S.byte_spans(tt, doc, ids, True)
        assert st == 0
        inside = [k for k, (s, e) in enumerate(sp) if s >= 1 and e <= len(doc) - 1 and e > s]
        if len(inside) < 2:
            continue
        found += 1
        chars = S.to_chars(doc, sp)
        assert all(chars[k] == (1, 2) for k in inside), (ch, sp, chars)
    assert found > 0


def test_empty_document_and_a_document_that_ends_in_an_unknown(oracle_mod):
    orc, is_byte = _oracle(oracle_mod, "VL")
    tt = S.TokenText(orc)
    assert S.byte_spans(tt, b"", [], is_byte) == ([], 0)
    assert S.spans(tt, b"", [], is_byte, "char") == ([], 0)
    rng = random.Random(1)
    for _ in range(400):
        doc = H.random_text(rng, max_words=6).encode("utf-8")
        ids, status = orc.encode_bytes(doc)
        if ids and ids[-1] == -1:
            sp = _check_properties(tt, doc, ids, status, is_byte)
            last = doc.decode("utf-8")[-1].encode("utf-8")
            assert sp[-1] == (len(doc) - len(last), len(doc))
            assert S.to_chars(doc, sp)[-1] == (len(doc.decode("utf-8")) - 1, len(doc.decode("utf-8")))
            return
    pytest.fail("no document ended in an id of -1")


def test_a_tampered_id_is_a_mismatch(oracle_mod):
    orc, is_byte = _oracle(oracle_mod, "VG")
    tt = S.TokenText(orc)
    doc = b"the quick brown fox jumps over the lazy dog"
    ids, _ = orc.encode_bytes(doc)
    assert S.byte_spans(tt, doc, ids, is_byte)[1] == 0
    bad = list(ids)
    bad[3] = ids[3] + 1 if ids[3] + 1 != ids[4] else ids[3] + 2
    assert S.byte_spans(tt, doc, bad, is_byte)[1] == S.MISMATCH


def test_batch_form_equals_the_per_document_form(oracle_mod):
    from hutoken_amd import synth
    orc, is_byte = _oracle(oracle_mod, "VG")
    tt = S.TokenText(orc)
    d, o = synth.corpus("C3", 6)
    ids, oo, _ = orc.encode_packed(d, o)
    for unit in ("byte", "char"):
        got, st = S.batch(tt, d, o, ids, oo, is_byte, unit, np.int64)
        assert not st.any() and got.dtype == np.int64 and got.shape == (len(ids), 2)
        raw = d.tobytes()
        for i in range(6):
            want, _ = S.spans(tt, raw[int(o[i]):int(o[i + 1])], ids[int(oo[i]):int(oo[i + 1])], is_byte, unit)
            assert got[int(oo[i]):int(oo[i + 1])].tolist() == [list(x) for x in want]


def test_library_exports_the_span_symbols():
    """(fails before the feature: the header did not declare them, the library did not export them)"""
    import os
    import re
    from hutoken_amd import _capi
    header = open(os.path.join(H.ROOT, "include", "hutoken_amd.h")).read()
    declared = set(re.findall(r"\b(hutk_[a-z0-9_]+)\s*\(", header))
    lib = _capi.load()
    for name in ("hutk_token_spans_device", "hutk_token_spans", "hutk_debug_span_tile_ids", "hutk_debug_span_chunk_bytes"):
        assert name in declared and name in _capi.EXPORTS and hasattr(lib, name), name
    for const, value in (("HUTK_SPANS_BYTES", 0), ("HUTK_SPANS_CHARS", 1)):
        assert re.search(r"#define %s %d\b" % (const, value), header)
    assert re.search(r"HUTK_DOC_SPAN_MISMATCH = 5\b", header)
    assert (_capi.SPANS_BYTES, _capi.SPANS_CHARS, _capi.DOC_SPAN_MISMATCH) == (0, 1, 5) == (0, 1, S.MISMATCH)
