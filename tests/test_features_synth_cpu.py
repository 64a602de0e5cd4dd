"""tests/features_synth.py held to its claims without a GPU: the bitmap and prefix counts of word_batch against a
bit-by-bit count, its expected ids against a hand-worked case and its bitmap against presplit_ref's word starts of a
real text; answers_fast against features_ref.answers; and every geometry case of tests/test_gpu_features_edges.py
against the property it is named for, from the arrays alone."""
import random

import numpy as np
import pytest

import features_ref as F
import features_synth as FS
import presplit_ref as SR


@pytest.fixture(scope="module")
def T():
    from hutoken_amd import _capi
    return _capi.word_ids_tile()


@pytest.fixture(scope="module")
def cases(T):
    return FS.word_cases(T)


def bit(batch, p):
    return (int(batch.bits[p >> 5]) >> (p & 31)) & 1


def check_arrays(b):
    """bits and before against a bit-by-bit count; shapes, padding, offsets"""
    assert b.bits.dtype == np.int32 and b.bits.shape == (b.n_bytes // 32 + 40,)
    assert b.before.dtype == np.int64 and b.before.shape == (b.n_bytes // 32 + 2,)
    want = set()
    for d in range(b.n_docs):
        want |= {int(b.text_offs[d]) + p for p in b.starts[d]}
    want.add(b.n_bytes)
    if b.junk:
        want |= set(range(b.lead)) | set(range(int(b.text_offs[-1]), b.n_bytes))
    count = 0
    for w in range(b.n_bytes // 32 + 40):
        if w < len(b.before):
            assert b.before[w] == count, w
        for i in range(32):
            p = 32 * w + i
            assert bit(b, p) == (p in want), p
            count += p in want
    assert b.text_offs[0] == b.lead and b.text_offs[-1] + b.tail == b.n_bytes and b.id_offs[0] == 0 and b.id_offs[-1] == b.n_ids
    assert b.spans.shape == (b.n_ids, 2) and b.words.shape == (b.n_ids,) and b.words.dtype == np.int32
    for d in range(b.n_docs):
        sp = b.spans[b.id_offs[d]:b.id_offs[d + 1]]
        assert (sp[:, 0] <= sp[:, 1]).all() and (sp >= 0).all() and (sp <= b.lens[d]).all()


def test_bitmap_and_prefix_counts_bit_by_bit(cases):
    for name in ("bit positions", "bit positions, lead 37, tail 50", "empty spans at a document's end", "edges, 3 empty", "no documents",
                 "no ids, 4 documents"):
        check_arrays(cases[name])
    check_arrays(FS.mismatch_base())
    plain = FS.word_batch([[[2], [3]]], lead=5, tail=4, junk=False)
    assert [p for p in range(64) if bit(plain, p)] == [5, 7, 14]
    junk = FS.word_batch([[[2], [3]]], lead=5, tail=4, junk=True)
    assert [p for p in range(64) if bit(junk, p)] == [0, 1, 2, 3, 4, 5, 7, 10, 11, 12, 13, 14]
    assert np.array_equal(plain.words, junk.words)


def test_hand_worked_ids():
    # "we'll see 12345" under gpt2: we | 'll | _see | _12345, tokens .. | _123 | 45; then an empty document and "ab" as a | b
    b = FS.word_batch([[[2], [3], [4], [4, 2]], [], [[1, 1]]], lead=1)
    assert b.text_offs.tolist() == [1, 16, 16, 18] and b.id_offs.tolist() == [0, 5, 5, 7] and b.n_bytes == 18
    assert b.spans.tolist() == [[0, 2], [2, 5], [5, 9], [9, 13], [13, 15], [0, 1], [1, 2]]
    assert b.words.tolist() == [0, 1, 2, 3, 3, 0, 0] and b.flagged == []
    assert [p for p in range(18 + 1) if bit(b, p)] == [0, 1, 3, 6, 10, 16, 18]
    assert b.before.tolist() == [0, 7]
    # the cl100k split of the same text: starts at bytes 10 and 13 as well, the first strictly inside the token (9, 13)
    c = FS.with_start(FS.with_start(b, 0, 10), 0, 13)
    assert c.words.tolist() == [0, 1, 2, 3, 5, 0, 0] and c.flagged == [0]
    c, flagged = FS.with_inner_start(b, 0, 3, "a+1")
    assert flagged == [0] and c.words.tolist() == [0, 1, 2, 3, 4, 0, 0]
    # empty spans: at a word's start, between two words (the next word's), at the document's end (the last word's)
    e = FS.word_batch([[[0, 2, 0], [1, 0]], [[1]]])
    assert e.spans.tolist() == [[0, 0], [0, 2], [2, 2], [2, 3], [3, 3], [0, 1]] and e.words.tolist() == [0, 0, 1, 1, 1, 0]


@pytest.mark.parametrize("preset", SR.PRESETS)
def test_bitmap_of_a_real_text(preset):
    doc = "we'll see 12345678 things!\n\n  ok 日本語".encode("utf-8")
    starts = SR.word_starts(doc, preset)
    edges = starts + [len(doc)]
    b = FS.word_batch([[[q - p] for p, q in zip(edges, edges[1:])]], lead=3, junk=False)
    packed = np.zeros(b.n_bytes // 32 + 40, dtype=np.uint32)
    for p in starts + [len(doc)]:
        packed[(p + 3) >> 5] |= np.uint32(1 << ((p + 3) & 31))
    assert np.array_equal(b.bits, packed.view(np.int32)) and b.starts[0] == starts
    assert b.words.tolist() == list(range(len(starts)))


# ---- answers ----------------------------------------------------------------------------------------------------------
def random_plan(rnd, spans_of_rows, cols):
    rows, at, flat = [], 0, []
    for i, (sp, col) in enumerate(zip(spans_of_rows, cols)):
        rows.append((i, 0, 0, 0, 0, at, len(sp), col))
        flat += sp.tolist()
        at += len(sp)
    return np.array(rows, dtype=np.int64), np.array(flat, dtype=np.int64).reshape(-1, 2)


def test_answers_fast_equals_features_ref():
    rnd = random.Random(8)
    for ks, n in (([rnd.randrange(1, 13) for _ in range(4000)], 4000), ([63] * 200, 200), ([64] * 200, 200), ([65] * 200, 200),
                  ([129] * 200, 200)):
        rows = [FS.span_rows(k, rnd.randrange(10 ** 9)) for k in ks]
        plan, spans = random_plan(rnd, rows, [rnd.randrange(0, 5) for _ in ks])
        ans = np.zeros((n, 2), dtype=np.int64)
        for i, sp in enumerate(rows):
            s = rnd.randrange(0, int(sp[-1, 1]) + 3)
            ans[i] = (s, s + rnd.randrange(1, 5)) if rnd.random() < 0.9 else (s, s - rnd.randrange(0, 2))
        want = F.answers(plan, "b", spans, ans)
        got = FS.answers_fast(plan, "b", spans, ans)
        assert got.dtype == want.dtype == np.int32 and np.array_equal(got, want)
        found = int((want[:, 0] >= 0).sum())
        assert n // 10 < found < n - n // 10, (ks[0], found)
        swapped = plan[:, [0, 1, 5, 6, 7, 2, 3, 4]]
        assert np.array_equal(FS.answers_fast(swapped, "a", spans, ans), want)
    assert FS.answers_fast(np.array([[0, 0, 0, 0, 0, 0, 0, 3]]), "b", np.zeros((0, 2)), np.array([[0, 1]])).tolist() == [[-1, -1]]


def test_span_rows_have_ties_overlaps_and_empty_spans():
    for k in (64, 129, 4098):
        sp = FS.span_rows(k, k)
        a, b = sp[:, 0], sp[:, 1]
        assert sp.shape == (k, 2) and (np.diff(a) >= 0).all() and (np.diff(b) >= 0).all() and (a <= b).all()
        assert (np.diff(a) == 0).any() and (np.diff(b) == 0).any() and (a == b).any() and (a[1:] < b[:-1]).any()
    assert FS.span_rows(1, 3).shape == (1, 2)


ANSWER_KS = (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 4098)


@pytest.mark.parametrize("k", ANSWER_KS)
def test_answer_cases_hold_found_and_not_found_rows(k):
    for side in ("a", "b"):
        plan, spans, ans = FS.answer_case(k, side)
        c = 2 if side == "a" else 5
        assert (plan[:, 0] == np.arange(len(plan))).all() and (plan[:, c] == 7).all() and (plan[:, c + 1] == k).all()
        assert len(spans) == 7 + k + 2 and len(ans) == len(plan)
        own = spans[7:7 + k]
        if k <= 129:
            assert len(plan) == 12 * k
            for j in range(k):
                for s in (own[j, 0] - 1, own[j, 0], own[j, 0] + 1):
                    for e in (s + 1, own[j, 1], own[-1, 1], own[-1, 1] + 1):
                        assert ((ans[:, 0] == s) & (ans[:, 1] == e)).any()
        else:
            js = {j for j in FS.BIG_J if j < k} | {k - 2, k - 1}
            assert len(plan) > 12 * 150 and all((ans[:, 0] == own[j, 0]).any() for j in js)
        want = FS.answers_fast(plan, side, spans, ans)
        found = int((want[:, 0] >= 0).sum())
        assert found * 10 >= len(plan) and (len(plan) - found) * 10 >= len(plan), (k, found, len(plan))
        # many different tokens are found, so not only those a round's 64 probes fall on; beyond 4096 where there are any
        for c in (0, 1):
            assert len(set(want[want[:, c] >= 0, c].tolist())) >= min(k, 150) // 3
        if k > 4096:
            assert (want[:, 0] - 3 >= 4096).any() and (want[:, 1] - 3 >= 4096).any()


# ---- word ids: the cases have the geometry they are named for -------------------------------------------------------
def first_ids(b):
    """the first id of every document that has ids"""
    return b.id_offs[:-1][np.diff(b.id_offs) > 0]


@pytest.mark.parametrize("empties", [0, 1, 3])
def test_documents_start_on_every_edge(cases, T, empties):
    b = cases["edges, %d empty" % empties]
    firsts = set(first_ids(b).tolist())
    wave = T // 4
    assert {T - 1, T, T + 1, 2 * T, wave - 1, wave, wave + 1} <= firsts and wave % (64 * FS.PER_THREAD) == 0
    inner = [f for f in firsts if wave + 8 < f < T - 8]
    assert sorted(f % FS.PER_THREAD for f in inner) == list(range(FS.PER_THREAD))
    assert len({f // FS.PER_THREAD for f in inner}) == FS.PER_THREAD  # each in the eight ids of another thread
    for f in FS.edge_firsts(T):  # `empties` empty documents at that same id, the one with ids behind them
        at = np.nonzero(b.id_offs[:-1] == f)[0]
        assert len(at) == empties + 1 and (np.diff(b.id_offs)[at[:-1]] == 0).all() and b.id_offs[at[-1] + 1] > f
    assert b.n_ids > 2 * T and not b.flagged


def test_many_starts_in_a_tile(cases, T):
    b = cases["3T one-token documents"]
    assert b.n_docs == b.n_ids == 3 * T and (np.diff(b.id_offs) == 1).all()
    b = cases["3T one-token documents, two empty behind each"]
    assert b.n_docs == 9 * T and b.n_ids == 3 * T
    for t in range(3):
        inside = ((b.id_offs[:-1] > t * T) & (b.id_offs[:-1] < (t + 1) * T)).sum()
        assert inside > 6000 and inside > 20 * 256  # the marking loop takes more than twenty trips
    for n in (256, 257, 513):
        b = cases["%d starts in tile 1" % n]
        assert ((b.id_offs[:-1] > T) & (b.id_offs[:-1] < 2 * T)).sum() == n
        assert 2 * T not in b.id_offs and b.id_offs[-1] > 2 * T  # the last of them runs into tile 2
        assert b.id_offs[1] > T  # tile 1 begins inside document 0: d0 = 0, the marks are 1 .. n


def test_runs_of_empty_documents(cases, T):
    b = cases["runs of empties"]
    lens = np.diff(b.id_offs)
    assert (lens[:T + 3] == 0).all() and lens[T + 3] == T  # more than T at the very front
    run = np.nonzero(b.id_offs[:-1] == T)[0]
    assert len(run) == T + 4 and (lens[run[:-1]] == 0).all() and lens[run[-1]] == 300  # the run ends exactly on id T
    mid = np.nonzero(b.id_offs[:-1] == T + 300)[0]
    assert len(mid) == 701 and lens[mid[-1]] == 50  # 700 marks on one id in the middle of tile 1
    assert (lens[-(T + 3):] == 0).all() and (b.id_offs[-(T + 4):] == b.n_ids).all()  # at the very end


def test_long_document_and_sizes(cases, T):
    b = cases["a long document"]
    assert b.id_offs.tolist() == [0, 5, 3 * T + 10, 3 * T + 17]  # tiles 1 and 2 hold no start
    assert cases["no ids, 4 documents"].n_ids == 0 and cases["no ids, 4 documents"].n_docs == 4
    assert cases["no documents"].n_docs == 0 and cases["no documents"].id_offs.tolist() == [0]
    for n in (1, T - 1, T, T + 1):
        assert cases["%d ids" % n].n_ids == n


def test_bit_positions(cases):
    for name in ("bit positions", "bit positions, lead 37, tail 50"):
        b = cases[name]
        assert {int(x) % 32 for x in b.text_offs[:-1]} == set(range(32))  # a document's text begins at every bit
        abs_starts = {int(b.text_offs[d]) + p for d in range(b.n_docs) for p in b.starts[d]}
        assert {p % 32 for p in abs_starts} >= {0, 31}
        abs_a = b.spans[:, 0] + np.repeat(b.text_offs[:-1], np.diff(b.id_offs))
        abs_b = b.spans[:, 1] + np.repeat(b.text_offs[:-1], np.diff(b.id_offs))
        size = abs_b - abs_a
        assert ((abs_a % 32 == 31) & (size >= 2)).any()  # a token whose first byte is the last of a bitmap word
        assert ((size == 100) & ((abs_b - 1) // 32 - abs_a // 32 == 3)).any()  # 100 bytes over four bitmap words
        firsts = {int(x) % 32 for x, n in zip(b.text_offs[:-1], b.lens) if n}
        assert {0, 31} <= firsts  # rank_excl at bit 0 and at bit 31 for a document's first byte
    a, c = cases["bit positions"], cases["bit positions, lead 37, tail 50"]
    assert np.array_equal(a.words, c.words) and c.lead == 37 and c.tail == 50 and c.junk
    assert all(bit(c, p) for p in range(37)) and all(bit(c, p) for p in range(c.n_bytes - 50, c.n_bytes + 1))
    e = cases["empty spans at a document's end"]
    ends = [d for d in range(e.n_docs) if e.lens[d] and (e.spans[e.id_offs[d + 1] - 1] == e.lens[d]).all()]
    assert len(ends) >= 4 and e.n_docs - 1 in ends  # ... the last document's too, in front of the junk of the tail
    for d in ends:
        assert e.words[e.id_offs[d + 1] - 1] == len(e.starts[d]) - 1  # the document's last word


def test_mismatch_cases():
    base = FS.mismatch_base()
    assert not base.flagged
    sp = base.doc_spans
    assert sp[1][1] == (1, 3) and sp[3][1] == (5, 45) and sp[4][1] == (2, 2) and sp[4][2] == (2, 3) and sp[1][2] == (3, 4)
    for where, doc, token in FS.MISMATCHES:
        b, flagged = FS.with_inner_start(base, doc, token, where)
        assert flagged == [doc]
        new = [p for p in b.starts[doc] if p not in base.starts[doc]]
        a, e = sp[doc][token]
        assert len(new) == 1 and a < new[0] < e
        assert new[0] == {"a+1": a + 1, "b-1": e - 1}.get(where, new[0])
        if where == "next":  # in the bitmap word behind the one that holds a, and not the token's last byte
            base_off = int(b.text_offs[doc])
            assert (base_off + new[0]) // 32 == (base_off + a) // 32 + 1 and new[0] < e - 1
        assert not np.array_equal(b.words, base.words)  # the ids behind the new start count one word more
    for _name, doc, pos in FS.CONTROLS:
        b = FS.with_start(base, doc, pos)
        assert not b.flagged and not np.array_equal(b.words, base.words)
        assert all(not (a < pos < e) for a, e in sp[doc])
    both, flagged = FS.with_inner_start(FS.with_inner_start(base, 1, 1, "a+1")[0], 3, 1, "b-1")
    assert flagged == [1, 3]


def test_foreign_spans(cases):
    b = cases["edges, 1 empty"]
    made = FS.foreign_spans(b)
    assert [n for n, _k, _s in made] == ["a = -1", "b = a - 1", "b = doc_len + 1"]
    for name, k, spans in made:
        diff = np.nonzero((spans != b.spans).any(axis=1))[0]
        assert diff.tolist() == [k]
        d = int(np.searchsorted(b.id_offs, k, side="right")) - 1
        a, e = spans[k].tolist()
        assert (a == -1) if name == "a = -1" else (e == a - 1 and a >= 0) if name == "b = a - 1" else (e == b.lens[d] + 1 and a >= 0)
