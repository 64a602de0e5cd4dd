"""The batches of tests/view_cases.py are what they claim to be, so that no test of tests/test_gpu_views.py passes
vacuously: chunk states by the normaliser's own rule, sizes and short edge tokens of the span batch, the piece boundaries
of the special-token batch, the places of the table ids.  No GPU."""
import importlib

import numpy as np
import pytest

import decode_ref as DR
import fallback_ref as F
import helpers as H
import norm_ref as R
import spans_ref as S
import specials_ref as SR
import view_cases as V

tables = importlib.import_module("hutoken_amd.normalize")


def _chunk():
    from hutoken_amd import _capi
    return _capi.norm_chunk_bytes()


def _oracle(oracle_mod, name):
    from hutoken_amd import data
    vp, sp, kw = data.vocab_files(name)
    return oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"]), kw["is_byte_encoder"]


def test_the_chunk_rule_restated():
    """chunk_states on hand-made text with a chunk of 8 bytes (NFC: lead 0xCC)"""
    offs = np.array([0, 20], dtype=np.int64)
    text = b"abcdefg\xc3\xa9jklmnop\xcc\x81st"  # C3 A9 straddles 8; CC is the first byte behind chunk 1 (no spill at 16)
    assert V.chunk_states(text, offs, 0xCC, 8) == [(True, 0), (False, 1), (False, 0)]
    assert V.chunk_states(text, offs, 0xC3, 8) == [(False, 0), (False, 1), (False, 0)]
    assert V.chunk_states(text, np.array([0, 8, 20]), 0xCC, 8)[1] == (False, 0)  # nothing spills over a document's end
    euro = b"abcdefg\xe2\x82\xacklmnopqr"
    assert V.chunk_states(euro, np.array([0, 18]), 0xCC, 8) == [(False, 0), (True, 2), (True, 0)]
    assert V.chunk_states(b"abcdefg\xe2\x82", np.array([0, 9]), 0xCC, 8)[1] == (True, 0)  # cut short: ill-formed, no spill


def test_the_clean_batch_is_clean_under_nfc():
    C = _chunk()
    docs = V.clean_docs(C)
    data, offs = R.pack(docs)
    assert len(data) >= 3 * C and all(R.norm_doc("NFC", d) == d for d in docs)
    assert (data >= 0x80).any()
    states = V.chunk_states(data, offs, tables.table_facts()["first_lead"][0], C)
    assert len(states) >= 4 and all(clean for clean, _sp in states)


@pytest.mark.parametrize("form", R.FORMS)
def test_clean_behind_dirty(form):
    C = _chunk()
    lead = tables.table_facts()["first_lead"][R.FORMS.index(form)]
    assert lead == {"NFC": 0xCC, "NFD": 0xC3, "NFKC": 0xC2, "NFKD": 0xC2}[form]
    sign = V.CHANGING[form][1]
    between = 1 if V.STRADDLE_CLEAN[form] else 0
    if V.STRADDLE_CLEAN[form]:
        b = V.STRADDLE_CLEAN[form].encode("utf-8")
        assert len(b) == 2 and 0xC2 <= b[0] < lead and R.norm_doc(form, b) == b
    else:
        assert lead == 0xC2  # no well-formed multi-byte character starts below it
    for ch in V.STRADDLE_FROM_DIRTY.values():
        assert all(R.norm_doc(f, ch.encode("utf-8")) == ch.encode("utf-8") for f in R.FORMS)
    cases = V.clean_behind_dirty_cases(form)
    assert {m for m, _s, _l in cases} == set(range(1, 17)) and {l for _m, _s, l in cases} == {1, 15, 16, 17, 40}
    assert {s for _m, s, _l in cases} == {0, 1, 2, 3}
    for m, sp, last in cases:
        for many in (False, True):
            docs, want = V.clean_behind_dirty(form, m, sp, last, C, many=many)
            data, offs = R.pack(docs)
            assert len(data) == 4 * C + last and (len(docs) == 1) == (not many)
            states = V.chunk_states(data, offs, lead, C)
            tag = (form, m, sp, last, many)
            assert len(states) == 5 and not states[0][0], tag
            assert all(clean for clean, _s in states[1:]), tag
            assert states[1][1] == sp, tag
            edge_spills = [s for _c, s in states[2:]]
            assert edge_spills == ([between if sp else 0, 0 if many else (between if sp else 0), between if sp else 0]), tag
            rd, ro, rc = R.reference(form, docs)
            assert len(rd) - len(data) == want == sign * m, tag
            assert (len(rd) - len(data)) % 16 == (sign * m) % 16 and rc[0] == 1 and not rc[1:].any(), tag
            if many:
                cuts = set(offs.tolist())
                assert {C + sp, 3 * C, 2 * C + 1} <= cuts and (np.diff(offs) == 0).any(), tag
                assert any(4 * C < c <= 4 * C + last for c in cuts), tag


@pytest.mark.parametrize("name", ["VG", "VL"])
def test_span_batch(oracle_mod, name):
    orc, is_byte = _oracle(oracle_mod, name)
    data, offs, ids, oo = V.spans_batch(orc)
    n = len(offs) - 1
    assert 2 * V.SPAN_CHUNK_BYTES < len(data) < 2 * V.SPAN_CHUNK_BYTES + 4096
    assert len(data) % 16 != 0 and len(ids) % V.SP_PER != 0 and len(ids) == oo[-1] and len(data) == offs[-1]
    assert offs[1] == 0 and offs[n - 1] == offs[n] and offs[2] > 0 and offs[n - 1] > offs[n - 2]  # empty first and last
    tt = S.TokenText(orc)
    raw = data.tobytes()
    for d in (1, n - 2):  # the first and the last document with text: short tokens at both of their ends
        doc = raw[int(offs[d]):int(offs[d + 1])]
        sp, st = S.byte_spans(tt, doc, ids[int(oo[d]):int(oo[d + 1])], is_byte)
        assert st == 0 and len(sp) >= 2
        first = next(x for x in sp if x[1] > x[0])  # (a stripped prefix alone is a first token of no bytes)
        assert sp[0][1] - sp[0][0] <= 7 and first[0] == 0 and first[1] <= 7, (name, d, sp[0], first)
        assert 1 <= sp[-1][1] - sp[-1][0] <= 7 and sp[-1][1] == len(doc), (name, d, sp[-1])
    assert raw[-1] < 0x80  # the byte the tampered case changes is a character of its own


def test_special_batch(oracle_mod):
    orc, _ = _oracle(oracle_mod, "VG")
    docs = V.special_batch(orc)
    specials = {V.EOT: V.EOT_ID}
    assert all(V.EOT in d for d in docs)
    data, offs = R.pack(docs)
    ids, oo, st, matches = SR.encode(orc, data, offs, specials)
    total = len(ids)
    assert 2 * V.CP_TILE < total < 2 * V.CP_TILE + 64 and total % 4 != 0 and not st.any() and matches >= len(docs)
    starts, tot = V.special_pieces(orc, docs, specials)
    assert tot == total
    assert ids[V.CP_TILE - 1] == V.EOT_ID and ids[V.CP_TILE] != V.EOT_ID  # a marker ends the tile, text begins the next
    k = starts.index(V.CP_TILE)
    assert starts[k + 1] > V.CP_TILE
    inside = [s for a, s, b in zip(starts, starts[1:], starts[2:] + [total]) if s % 4 and a < s < b]
    assert len(inside) > 100  # boundaries between two non-empty pieces inside a group of four


def test_fallback_decode_batch():
    ents, special = H.random_char_vocab(5, n_merges=400, drop_chars="őű漢")
    table = V.byte_table(ents)
    assert sorted(table.tolist()) == list(range(256))
    specials = [(b"<|eot|>", len(ents) + 5), (b"<s>", 300)]
    tokens = F.from_decode_ref(DR.DecodeRef(ents, special, "▁", False))
    for sp in ((), [i for _k, i in specials]):
        ids, offs = V.fallback_decode_batch(ents, table, sp)
        assert len(ids) == V.FBR_TILE + 1 == offs[-1] and offs[0] == 0 and (np.diff(offs) >= 0).all()
        in_table = np.isin(ids, table)
        assert set(np.nonzero(in_table)[0].tolist()) == set(V.FB_TABLE_AT)
        assert V.FBR_TILE in offs.tolist() and (np.diff(offs) == 0).any() and any(o % 4 for o in offs.tolist())
        out, oo, st = F.decode_packed(tokens, ids, offs, table, specials if sp else None)
        assert not st.any() and oo[-1] > V.FBR_TILE
        if sp:
            assert np.isin(ids, sp).any()


def test_collate_batch():
    ids, offs = V.collate_batch()
    lens = np.diff(offs)
    assert len(lens) == 300 and lens.min() == 0 and lens.max() == 40 and (ids < 0).any() and V.COLLATE_L % 4 == 0
    half = 150
    assert int(offs[half]) % V.COLLATE_L != 0  # a row straddles the two add calls of the packer
