"""Row-aligned features without a GPU: the plain restatement of tests/features_ref.py against the three collation
references (rebuilding input_ids from plan + ids + template), the closed-form answer rule against run_qa's while-loops,
hand-worked word ids, the texts the GPU tests rely on, and every argument check of the Python surface and the C ABI that
needs no device.  The kernels are compared with the restatement in tests/test_gpu_features.py."""
import random

import numpy as np
import pytest

import collate_ref as CR
import features_cases as FC
import features_ref as F
import pairs_ref as PR
import presplit_ref as SR
import spans_ref as S
import windows_ref as WR

import hutoken_amd
from hutoken_amd import _capi

NO = _capi.NO_TOKEN
C_NAMES = ("hutk_padded_plan_device", "hutk_windows_plan_device", "hutk_pair_plan_device", "hutk_rows_gather_device",
           "hutk_token_word_ids_device", "hutk_rows_answers_device", "hutk_debug_word_ids_tile")
PY_NAMES = ("gather_rows", "answer_positions", "token_word_ids_device")


def same(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)


# ---- plans: rebuilding the rows of the three references -------------------------------------------------------------
def test_padded_plans_rebuild_the_reference_rows():
    rng = random.Random(6)  # (the generator of test_collate_cpu.test_vectorised_forms_equal_the_loop_forms)
    for trial in range(150):
        docs = [[rng.randint(-3, 50) for _ in range(rng.choice([0, 0, 1, 2, 3, rng.randint(0, 30)]))] for _ in range(rng.randint(0, 40))]
        ids, offs = CR.ragged(docs)
        kw = rng.choice([{}, {"eos_id": 99}, {"bos_id": 98, "eos_id": 99}, {"bos_id": 98}])
        dtype = rng.choice([np.int32, np.int64])
        L = max(rng.choice([1, 2, 3, 4, 7, 16, 64]), len(kw))
        for tr in ("right", "left"):
            for side in ("right", "left"):
                want = CR.padded(ids, offs, L, pad_id=-7, truncation=tr, padding_side=side, dtype=dtype, **kw)
                plan = F.padded_plan(offs, L, truncation=tr, padding_side=side, **kw)
                assert same(F.rebuild(plan, L, ids, pad_id=-7, dtype=dtype, **kw), want[0]), (trial, docs, L, kw, tr, side)
                assert np.array_equal(plan[:, 3] + len(kw), want[2]) and np.array_equal(plan[:, 0], np.arange(len(docs)))
                assert not plan[:, 5:7].any() and np.array_equal(plan[:, 7], plan[:, 4] + plan[:, 3])
                if tr == "right":
                    assert not plan[:, 1].any()


def test_windows_plans_rebuild_the_reference_rows():
    rnd = random.Random(5)  # (the generator of test_windows_cpu.test_vectorised_form_equals_the_loop_form)
    for trial in range(150):
        docs = [[rnd.randrange(-3, 1000) for _ in range(rnd.choice((0, 1, 2, 3, 5, 8, 13, 40)))] for _ in range(rnd.randrange(0, 9))]
        ids, offs = WR.ragged(docs)
        kw = rnd.choice(({}, {"eos_id": 99}, {"bos_id": -5}, {"bos_id": -5, "eos_id": 99}))
        L = rnd.randrange(len(kw) + 1, 12)
        stride = rnd.randrange(0, L - len(kw))
        for side in ("right", "left"):
            want = WR.windows(ids, offs, L, stride, pad_id=-7, padding_side=side, **kw)
            plan = F.windows_plan(offs, L, stride, padding_side=side, **kw)
            label = (trial, docs, L, stride, kw, side)
            assert same(F.rebuild(plan, L, ids, pad_id=-7, **kw), want[0]), label
            assert np.array_equal(plan[:, :2], want[3]) and np.array_equal(plan[:, 3] + len(kw), want[2]), label


def test_pair_plans_rebuild_the_reference_rows():
    rnd = random.Random(5)  # (the generator of test_pairs_cpu.test_vectorised_forms_equal_the_loop_forms)
    for trial in range(200):
        n = rnd.randrange(0, 9)
        lens = (0, 1, 2, 3, 5, 8, 13, 40)
        docs_a = [[rnd.randrange(-3, 1000) for _ in range(rnd.choice(lens))] for _ in range(n)]
        docs_b = [[rnd.randrange(-3, 1000) for _ in range(rnd.choice(lens))] for _ in range(n)]
        a, oa = PR.ragged(docs_a, base=rnd.choice((0, 0, 3)), tail=rnd.choice((0, 2)))
        b, ob = PR.ragged(docs_b, base=rnd.choice((0, 1, 7)))
        if trial % 4 == 0:  # both sides in one ids array, B's offsets a view with a non-zero base
            a, oo = PR.ragged(docs_a + docs_b, base=rnd.choice((0, 2)))
            b, oa, ob = a, oo[:n + 1], oo[n:]
        kw = {"sep_ids": tuple(rnd.randrange(-9, 99) for _ in range(trial % 5))}
        if rnd.random() < 0.5:
            kw["bos_id"] = -5
        if rnd.random() < 0.5:
            kw["eos_id"] = 99
        s = len(kw["sep_ids"]) + len(kw) - 1
        L = rnd.randrange(s + 1, s + 14)
        stride = rnd.randrange(0, L - s)
        for side in ("right", "left"):
            for strategy in PR.STRATEGIES:
                label = (trial, docs_a, docs_b, L, stride, kw, side, strategy)
                want = PR.pairs(a, oa, b, ob, L, strategy, pad_id=-7, padding_side=side, **kw)
                plan = F.pairs_plan(oa, ob, L, strategy, padding_side=side, **kw)
                assert same(F.rebuild(plan, L, a, b, pad_id=-7, **kw), want[0]), label
                assert np.array_equal(plan[:, 3] + plan[:, 6] + s, want[3]), label
                # the token types are 1 from the B side's first column to the row's end
                types = np.zeros_like(want[2])
                for r, row in enumerate(plan.tolist()):
                    types[r, row[7]:row[4] - ("bos_id" in kw) + want[3][r]] = 1
                assert same(types, want[2]), label
                if strategy == "longest_first":
                    continue
                want = PR.pair_windows(a, oa, b, ob, L, stride, strategy, pad_id=-7, padding_side=side, **kw)
                plan = F.pair_windows_plan(oa, ob, L, stride, strategy, padding_side=side, **kw)
                assert same(F.rebuild(plan, L, a, b, pad_id=-7, **kw), want[0]), label
                assert np.array_equal(plan[:, :2], want[4]) and np.array_equal(plan[:, 3] + plan[:, 6] + s, want[3]), label


def test_kept_lengths_by_the_loop_equal_the_closed_form():
    for strategy in PR.STRATEGIES:
        for R in range(1, 9):
            for na in range(0, 12):
                for nb in range(0, 12):
                    assert F.kept(na, nb, R, strategy) == PR.pair_lengths(na, nb, R, strategy), (strategy, R, na, nb)


def test_worked_plans():
    # three ids of room: a document of 5 ids in windows of stride 1, with bos and eos, padded on the left
    plan = F.windows_plan(np.array([0, 5, 5, 7]), 5, 1, bos_id=1, eos_id=2, padding_side="left")
    assert plan.tolist() == [[0, 0, 0, 3, 1, 0, 0, 4], [0, 2, 2, 3, 1, 0, 0, 4], [1, 0, 5, 0, 4, 0, 0, 4], [2, 0, 5, 2, 2, 0, 0, 4]]
    # a question of 2 ids and a context of 5 in rows of 8 with bos, one separator and eos: C = 3
    plan = F.pair_windows_plan(np.array([0, 2]), np.array([2, 7]), 8, 1, "only_second", bos_id=1, sep_ids=(4,), eos_id=2)
    assert plan.tolist() == [[0, 0, 0, 2, 1, 2, 3, 4], [0, 2, 0, 2, 1, 4, 3, 4]]
    plan = F.padded_plan(np.array([0, 6]), 4, eos_id=2, truncation="left")
    assert plan.tolist() == [[0, 3, 3, 3, 0, 0, 0, 3]]


# ---- answers: the closed form against run_qa's loops ----------------------------------------------------------------
def run_qa_positions(offsets, first, last, start_char, end_char):
    """prepare_train_features of the question-answering example (run_qa.py), its two while-loops bounded to the window's
    own tokens first .. last (there the neighbours are special tokens whose offsets stop the loops; here nothing is
    read behind the window)."""
    token_start_index, token_end_index = first, last
    if not (offsets[token_start_index][0] <= start_char and offsets[token_end_index][1] >= end_char):
        return -1, -1
    while token_start_index <= last and offsets[token_start_index][0] <= start_char:
        token_start_index += 1
    while token_end_index >= first and offsets[token_end_index][1] >= end_char:
        token_end_index -= 1
    return token_start_index - 1, token_end_index + 1


def test_closed_form_answers_equal_the_run_qa_loops():
    rnd = random.Random(8)
    found = cases = 0
    for _trial in range(4000):
        k = rnd.randrange(1, 12)
        at, spans = rnd.randrange(0, 4), []
        last_b = 0
        for _ in range(k):  # starts and ends both non-decreasing, with ties, overlaps and empty spans among them
            a = at + rnd.choice((0, 0, 0, 1))
            b = max(last_b, a + rnd.choice((0, 1, 1, 2, 3)))
            spans.append((a, b))
            last_b = b
            at = b if rnd.random() < 0.8 else a
        col = rnd.randrange(0, 5)
        s = rnd.randrange(0, at + 3)
        e = s + rnd.randrange(1, 5)
        want = run_qa_positions(spans, 0, k - 1, s, e)
        want = (col + want[0], col + want[1]) if want[0] >= 0 else want
        assert F.answer(spans, col, s, e) == want, (spans, col, s, e)
        cases += 1
        found += want[0] >= 0
    assert cases == 4000 and 1000 < found < 3500
    assert F.answer([(0, 2), (2, 5)], 3, -1, -1) == (-1, -1) and F.answer([], 3, 0, 1) == (-1, -1)
    assert F.answer([(0, 2), (2, 5)], 3, 4, 4) == (-1, -1)  # s >= e: none
    assert F.answer([(0, 2), (2, 5), (5, 9)], 3, 2, 5) == (4, 4) and F.answer([(0, 2), (2, 5), (5, 9)], 3, 1, 6) == (3, 5)
    assert F.answer([(0, 2), (2, 5), (5, 9)], 3, 5, 10) == (-1, -1)  # the answer ends behind the window


# ---- word ids ---------------------------------------------------------------------------------------------------------
def test_hand_worked_word_ids():
    doc = b"we'll see 12345"
    gpt2, cl100k = SR.word_starts(doc, "gpt2"), SR.word_starts(doc, "cl100k")
    assert gpt2 == [0, 2, 5, 9]  # we | 'll | _see | _12345
    assert cl100k == [0, 2, 5, 9, 10, 13]  # we | 'll | _see | _ | 123 | 45
    under_gpt2 = [(0, 2), (2, 5), (5, 9), (9, 13), (13, 15)]  # .. | _123 | 45
    under_cl100k = [(0, 2), (2, 5), (5, 9), (9, 10), (10, 13), (13, 15)]
    assert F.word_ids(doc, under_gpt2, gpt2) == ([0, 1, 2, 3, 3], False)
    assert F.word_ids(doc, under_cl100k, cl100k) == ([0, 1, 2, 3, 4, 5], False)
    assert F.word_ids(doc, under_gpt2, cl100k) == ([0, 1, 2, 3, 5], True)  # 10 lies strictly inside (9, 13)
    assert F.word_ids(doc, under_cl100k, gpt2) == ([0, 1, 2, 3, 3, 3], False)  # a finer split of the same words
    # byte-level tokens that split a character: both halves belong to the character's word; an empty span never mismatches
    doc = "a é".encode("utf-8")
    assert SR.word_starts(doc, "gpt2") == [0, 1]
    assert F.word_ids(doc, [(0, 1), (1, 3), (3, 4), (4, 4)], [0, 1]) == ([0, 1, 1, 1], False)
    assert F.word_ids(b"", [], []) == ([], False)


def test_the_chosen_texts_encode_without_unknown_ids_or_mismatches(oracle_mod):
    """What tests/test_gpu_features.py relies on: VG is byte-level, so on these texts no id is -1 and spans_ref finds every
    token's bytes where its span lies."""
    from hutoken_amd import data
    vp, sp, kw = data.vocab_files("VG")
    orc = oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"])
    tt = S.TokenText(orc)
    texts = FC.QUESTIONS + FC.CONTEXTS + FC.NER_TEXTS + FC.short_texts() + [FC.long_text(3000)]
    for t in texts:
        doc = t.encode("utf-8")
        ids, status = orc.encode_bytes(doc)
        assert status == 0 and -1 not in ids, t
        spans, st = S.byte_spans(tt, doc, ids, kw["is_byte_encoder"])
        assert st == 0 and (not spans or (spans[0][0] == 0 and spans[-1][1] == len(doc))), t
        for preset in ("gpt2", "cl100k"):
            starts = SR.word_starts(doc, preset)
            assert (starts[:1] == [0]) == bool(doc), t  # a word starts at the first byte of every document that has one
    orc.close()


# ---- the Python surface: argument checks come before any device call ------------------------------------------------
def test_names_are_exported():
    for name in PY_NAMES:
        assert name in hutoken_amd.__all__ and callable(getattr(hutoken_amd, name))
    for name in C_NAMES:
        assert name in _capi.EXPORTS
        assert hasattr(_capi.load(), name) and getattr(_capi.load(), name).argtypes is not None
    assert _capi.word_ids_tile() > 0 and _capi.word_ids_tile() % 256 == 0


def host_plan(n=2):
    import torch
    return torch.zeros((n, 8), dtype=torch.int64)


def test_gather_rows_argument_checks():
    import torch
    plan, vals = host_plan(), torch.zeros(5, dtype=torch.int32)
    pairs = torch.zeros((5, 2), dtype=torch.int64)
    for bad in ([[0] * 8], None, np.zeros((2, 8), dtype=np.int64)):
        with pytest.raises(TypeError, match="row_plan"):
            hutoken_amd.gather_rows(bad, 4, vals)
    with pytest.raises(TypeError, match="int64"):
        hutoken_amd.gather_rows(plan.to(torch.int32), 4, vals)
    for bad in (torch.zeros((2, 7), dtype=torch.int64), torch.zeros(16, dtype=torch.int64), torch.zeros((2, 16), dtype=torch.int64)[:, ::2]):
        with pytest.raises(ValueError, match="row_plan"):
            hutoken_amd.gather_rows(bad, 4, vals)
    for bad in (0, -1, 2**31):
        with pytest.raises(ValueError, match="max_length"):
            hutoken_amd.gather_rows(plan, bad, vals)
    for bad in (4.0, True, None):
        with pytest.raises(TypeError, match="max_length"):
            hutoken_amd.gather_rows(plan, bad, vals)
    with pytest.raises(TypeError, match="values_a"):
        hutoken_amd.gather_rows(plan, 4, [1, 2, 3])
    for bad in (vals.to(torch.int16), vals.to(torch.float32), vals.to(torch.uint8)):
        with pytest.raises(TypeError, match="values_a"):
            hutoken_amd.gather_rows(plan, 4, bad)
    for bad in (torch.zeros((5, 3), dtype=torch.int32), torch.zeros((5, 2, 1), dtype=torch.int32), torch.zeros(10, dtype=torch.int32)[::2],
                torch.zeros((), dtype=torch.int32)):
        with pytest.raises(ValueError, match="values_a"):
            hutoken_amd.gather_rows(plan, 4, bad)
    for bad in (pairs, vals.to(torch.int64), torch.zeros((5, 2), dtype=torch.int32)):
        with pytest.raises(TypeError, match="values_b"):
            hutoken_amd.gather_rows(plan, 4, vals, bad)
    for bad in (1.5, "0", True, (1, 2.0), None):
        with pytest.raises(TypeError, match="fill"):
            hutoken_amd.gather_rows(plan, 4, pairs, fill=bad)
    for bad in ((1, 2), (1, 2, 3), ()):
        with pytest.raises(ValueError, match="fill"):
            hutoken_amd.gather_rows(plan, 4, vals, fill=bad)
    with pytest.raises(ValueError, match="fill"):
        hutoken_amd.gather_rows(plan, 4, pairs, fill=(1, 2, 3))
    with pytest.raises(ValueError, match="fit int32"):
        hutoken_amd.gather_rows(plan, 4, vals, fill=2**31)
    with pytest.raises(ValueError, match="fit int64"):
        hutoken_amd.gather_rows(plan, 4, pairs, fill=(0, -2**63 - 1))
    # sound arguments on the host: refused for where they are, not computed there
    for args, kw in (((plan, 4, vals), {}), ((plan, 4, pairs), {"fill": (0, 0)}), ((plan, 4, pairs, pairs), {"fill": -1}),
                     ((plan, 4, vals, vals), {"fill": 2**31 - 1})):
        with pytest.raises(ValueError, match="on the GPU"):
            hutoken_amd.gather_rows(*args, **kw)


def test_answer_positions_argument_checks():
    import torch
    plan = host_plan()
    spans, answers = torch.zeros((5, 2), dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int64)
    with pytest.raises(TypeError, match="row_plan"):
        hutoken_amd.answer_positions(None, spans, answers)
    with pytest.raises(ValueError, match="row_plan"):
        hutoken_amd.answer_positions(torch.zeros((2, 2), dtype=torch.int64), spans, answers)
    with pytest.raises(TypeError, match="spans"):
        hutoken_amd.answer_positions(plan, [(0, 1)], answers)
    with pytest.raises(TypeError, match="spans"):
        hutoken_amd.answer_positions(plan, spans.to(torch.float32), answers)
    for bad in (torch.zeros(5, dtype=torch.int32), torch.zeros((5, 3), dtype=torch.int32)):
        with pytest.raises(ValueError, match="spans"):
            hutoken_amd.answer_positions(plan, bad, answers)
    with pytest.raises(TypeError, match="answers"):
        hutoken_amd.answer_positions(plan, spans, [(0, 1), (2, 3)])
    with pytest.raises(ValueError, match="answers"):
        hutoken_amd.answer_positions(plan, spans, torch.zeros(4, dtype=torch.int64))
    for bad in ("c", "B", 1, None):
        with pytest.raises(ValueError, match="side"):
            hutoken_amd.answer_positions(plan, spans, answers, side=bad)
    for side in ("a", "b"):
        with pytest.raises(ValueError, match="on the GPU"):
            hutoken_amd.answer_positions(plan, spans, answers, side=side)


def test_return_plan_changes_no_argument_check():
    import torch
    ids, offs = torch.tensor([1, 2, 3], dtype=torch.int32), torch.tensor([0, 1, 3], dtype=torch.int64)
    for rp in (False, True):
        with pytest.raises(ValueError, match="on the GPU"):
            hutoken_amd.collate_padded(ids, offs, 4, return_plan=rp)
        with pytest.raises(ValueError, match="on the GPU"):
            hutoken_amd.collate_windows(ids, offs, 4, 1, return_plan=rp)
        with pytest.raises(ValueError, match="on the GPU"):
            hutoken_amd.collate_pairs(ids, offs, ids, offs, 4, return_plan=rp)
        with pytest.raises(ValueError, match="on the GPU"):
            hutoken_amd.collate_pair_windows(ids, offs, ids, offs, 4, 1, return_plan=rp)
        with pytest.raises(ValueError, match="stride"):
            hutoken_amd.collate_windows(ids, offs, 4, 4, return_plan=rp)


def test_text_entry_points_check_their_feature_arguments(monkeypatch):
    calls = (lambda **kw: hutoken_amd.batch_encode_padded(["a"], 8, **kw),
             lambda **kw: hutoken_amd.batch_encode_windows(["a"], 8, 2, **kw),
             lambda **kw: hutoken_amd.batch_encode_pairs(["a"], ["b"], 8, **kw),
             lambda **kw: hutoken_amd.batch_encode_pair_windows(["a"], ["b"], 8, 2, **kw))
    monkeypatch.setattr(hutoken_amd, "_ctx", None)
    for call in calls:
        with pytest.raises(TypeError, match="return_offsets_mapping"):
            call(return_offsets_mapping=1)
        with pytest.raises(TypeError, match="return_word_ids"):
            call(return_word_ids="yes")
        with pytest.raises(ValueError, match="unit"):
            call(return_offsets_mapping=True, offsets_unit="word")
        with pytest.raises(RuntimeError, match="initialize"):
            call(return_offsets_mapping=True, return_word_ids=True)
    import torch
    t = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="initialize"):
        hutoken_amd.token_word_ids_device(t, t, t, t)

    class NoPreset:  # a context with the built-in splitter: nothing is encoded before word ids are refused
        pretokenizer = None
    monkeypatch.setattr(hutoken_amd, "_ctx", NoPreset())
    for call in calls:
        with pytest.raises(ValueError, match="split preset"):
            call(return_word_ids=True)
    with pytest.raises(ValueError, match="split preset"):
        hutoken_amd.token_word_ids_device(t, t, t, t)
    with pytest.raises(ValueError, match="preset"):
        hutoken_amd.token_word_ids_device(t, t, t, t, preset="o200k")
    with pytest.raises(TypeError, match="preset"):
        hutoken_amd.token_word_ids_device(t, t, t, t, preset=1)


# ---- the C ABI: what is refused before a device is looked for -------------------------------------------------------
def test_c_abi_argument_checks_need_no_device():
    L = _capi.load()
    E = _capi.E_ARG
    fill = (_capi.C.c_int32 * 4)()
    assert L.hutk_padded_plan_device(None, -1, 0, 8, NO, NO, 0, None, None, None) == E
    assert L.hutk_padded_plan_device(None, 0, 0, 0, NO, NO, 0, None, None, None) == E
    assert L.hutk_padded_plan_device(None, 0, 0, 1, 1, 2, 0, None, None, None) == E  # max_len below bos + eos
    assert L.hutk_padded_plan_device(None, 0, 0, 8, NO, NO, 4, None, None, None) == E  # an unknown flag
    assert L.hutk_windows_plan_device(None, None, 0, 0, 0, 8, 8, NO, NO, 0, None, None, None) == E  # stride >= C
    assert L.hutk_windows_plan_device(None, None, 0, 0, 0, 2, 0, 1, 2, 0, None, None, None) == E  # no room
    assert L.hutk_windows_plan_device(None, None, 0, 0, 0, 8, 0, NO, NO, _capi.COLLATE_TRUNC_LEFT, None, None, None) == E
    assert L.hutk_windows_plan_device(None, None, 0, 0, -1, 8, 0, NO, NO, 0, None, None, None) == E
    sep = (_capi.C.c_int32 * 4)(4, 5, NO, 7)
    pair = lambda *a: L.hutk_pair_plan_device(None, None, None, *a, None, None, None)  # noqa: E731
    assert pair(0, 0, 0, 0, 8, 0, 3, NO, sep, 0, NO, 0) == E  # an unknown strategy
    assert pair(0, 0, 0, 0, 8, 0, 0, NO, sep, 5, NO, 0) == E  # five separators
    assert pair(0, 0, 0, 0, 8, 0, 0, NO, sep, 3, NO, 0) == E  # an absent id among them
    assert pair(0, 0, 0, 0, 3, 0, 0, 1, sep, 2, 2, 0) == E  # no room
    assert pair(0, 0, 0, 0, 8, 7, 0, NO, sep, 1, NO, 0) == E  # stride >= R
    assert pair(2, 0, 0, 3, 8, 0, 0, NO, sep, 1, NO, 0) == E  # one row per pair: n_rows must be n_pairs
    assert pair(0, 0, 0, 0, 8, 0, 0, NO, sep, 1, NO, 1) == E  # HUTK_COLLATE_TRUNC_LEFT does not apply
    for rec in (0, 2, 12, 32):
        assert L.hutk_rows_gather_device(None, 0, 8, None, 0, None, 0, rec, fill, None, None, None) == E
    assert L.hutk_rows_gather_device(None, 0, 0, None, 0, None, 0, 4, fill, None, None, None) == E
    assert L.hutk_rows_gather_device(None, 0, 2**31, None, 0, None, 0, 4, fill, None, None, None) == E
    assert L.hutk_rows_gather_device(None, -1, 8, None, 0, None, 0, 4, fill, None, None, None) == E
    assert L.hutk_rows_gather_device(None, 0, 8, None, 0, None, 0, 4, None, None, None, None) == E  # no fill record
    for side, width in ((2, 4), (-1, 4), (0, 2), (1, 16)):
        assert L.hutk_rows_answers_device(None, 0, side, None, width, 0, None, 0, None, None, None) == E
    assert L.hutk_rows_answers_device(None, -1, 0, None, 4, 0, None, 0, None, None, None) == E
    for width in (0, 2, 16):
        assert L.hutk_token_word_ids_device(None, None, None, 0, 0, None, width, None, 0, None, None, None, None) == E
    assert L.hutk_token_word_ids_device(None, None, None, -1, 0, None, 4, None, 0, None, None, None, None) == E
    assert "span_width" in _capi.last_error()


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the calls would run")
    L = _capi.load()
    fill = (_capi.C.c_int32 * 4)()
    assert L.hutk_padded_plan_device(None, 0, 0, 8, NO, NO, 0, None, None, None) == _capi.E_DEVICE
    assert L.hutk_rows_gather_device(None, 0, 8, None, 0, None, 0, 4, fill, None, None, None) == _capi.E_DEVICE
    assert L.hutk_rows_answers_device(None, 0, 1, None, 4, 0, None, 0, None, None, None) == _capi.E_DEVICE
    assert L.hutk_token_word_ids_device(None, None, None, 0, 0, None, 4, None, 0, None, None, None, None) == _capi.E_DEVICE
